#!/usr/bin/env python3
"""Writes tests/golden/gpt_*.npz: the reference's GPT_Backbone (robomimic/models/transformers.py) on the CPU, on seeded inputs.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_gpt.py --ref <reference checkout>

transformers.py is loaded by file path.  It imports robomimic.models.base_nets (for `Module`), robomimic.utils.tensor_utils
and robomimic.utils.torch_utils, whose real versions pull in packages this project does not need; stub modules stand in for
them in sys.modules (`Module` = nn.Module, which is all the backbone uses of them).  Nothing of the reference is copied: a
fixture holds arrays only (no pickles) --
    seed, B, L, E, H, layers, causal      the case; dropout probabilities are 0 everywhere
    x                                     inputs [B, L, E], drawn from torch.Generator().manual_seed(seed + 1)
    out32, out64                          the module's fp32 output and the output of its .double() copy on x.double()
    gx32, gx64                            d L / d x for L = sum(out * r), r = tests/gpt_ref.objective_weights(seed, shape)
    gp32/<name>, gp64/<name>              d L / d parameter for the parameters of tests/gpt_ref.STORED_PARAM_GRADS and the first
                                          rows of STORED_WEIGHT_ROWS
    dev/out, dev/gx, dev/gp/<name>        max |fp32 - fp64| / max |fp64| of each of the above: the fp32 reference's own error
    keys, shapes                          the state_dict's keys in order and their shapes (padded with -1 to 4 dimensions)
    params_sha256                         tests/gpt_ref.state_hash of the state_dict after torch.manual_seed(seed) + construction
Parameters are NOT stored: tests re-draw them by constructing the module under the same seed.
"""
import argparse
import copy
import importlib.util
import io
import sys
import types
from contextlib import redirect_stdout
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import gpt_ref  # noqa: E402

CASES = {                     # name: (seed, B, L, E, H, layers, causal)
    "gpt_icrt": (601, 2, 30, 512, 8, 6, True),
    "gpt_small": (602, 3, 12, 64, 4, 2, True),
    "gpt_noncausal": (603, 2, 12, 64, 4, 2, False),
    "gpt_len3": (604, 2, 3, 128, 2, 2, True),
}


def load_reference(ref: Path):
    for name in ("robomimic", "robomimic.models", "robomimic.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    base = types.ModuleType("robomimic.models.base_nets")
    base.Module = nn.Module
    sys.modules["robomimic.models.base_nets"] = base
    for name in ("tensor_utils", "torch_utils"):
        m = types.ModuleType("robomimic.utils." + name)
        sys.modules["robomimic.utils." + name] = m
        setattr(sys.modules["robomimic.utils"], name, m)
    spec = importlib.util.spec_from_file_location("ref_transformers", ref / "robomimic" / "models" / "transformers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


def run_case(tf, name, seed, B, L, E, H, layers, causal, out_dir):
    torch.manual_seed(seed)
    with redirect_stdout(io.StringIO()):
        net = tf.GPT_Backbone(embed_dim=E, context_length=L, causal=causal, attn_dropout=0.0, block_output_dropout=0.0,
                              num_layers=layers, num_heads=H)
    net.eval()
    sd = net.state_dict()
    x = torch.randn(B, L, E, generator=torch.Generator().manual_seed(seed + 1))
    r = gpt_ref.objective_weights(seed, (B, L, E))
    last = layers - 1
    names = [n.format(last=last) for n in gpt_ref.STORED_PARAM_GRADS]

    def run(module, xin, rin):
        module.zero_grad()
        xin = xin.clone().requires_grad_(True)
        out = module(xin)
        (out * rin).sum().backward()
        p = dict(module.named_parameters())
        g = {n: p[n].grad.clone() for n in names}
        for n, rows in gpt_ref.STORED_WEIGHT_ROWS:
            g[f"{n}[:{rows}]"] = p[n].grad[:rows].clone()
        return out.detach(), xin.grad.clone(), g

    out32, gx32, gp32 = run(net, x, r)
    out64, gx64, gp64 = run(copy.deepcopy(net).double(), x.double(), r.double())

    # the restatement the tests use must BE the reference on this case, bit for bit
    xr = x.clone().requires_grad_(True)
    mine = gpt_ref.gpt_forward(sd, xr, layers, H)
    (mine * r).sum().backward()
    assert torch.equal(mine.detach(), out32) and torch.equal(xr.grad, gx32), "tests/gpt_ref.py drifted from the reference"

    keys = list(sd)
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    arrays = dict(seed=seed, B=B, L=L, E=E, H=H, layers=layers, causal=int(causal), x=x.numpy(), out32=out32.numpy(),
                  out64=out64.numpy(), gx32=gx32.numpy(), gx64=gx64.numpy(), keys=np.array(keys), shapes=shapes,
                  params_sha256=np.array(gpt_ref.state_hash(sd)))
    arrays["dev/out"], arrays["dev/gx"] = _rel(out32, out64), _rel(gx32, gx64)
    for n in gp32:
        arrays["gp32/" + n], arrays["gp64/" + n] = gp32[n].numpy(), gp64[n].numpy()
        arrays["dev/gp/" + n] = _rel(gp32[n], gp64[n])
    path = out_dir / f"{name}.npz"
    np.savez_compressed(path, **arrays)
    np.load(path, allow_pickle=False)["keys"]                           # arrays only: loads without pickle
    print(f"{name}: {path.stat().st_size} bytes, dev/out {arrays['dev/out']:.3e}, dev/gx {arrays['dev/gx']:.3e}, "
          f"max dev/gp {max(v for k, v in arrays.items() if k.startswith('dev/gp/')):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden"))
    a = ap.parse_args()
    torch.set_num_threads(1)               # one thread: the fp32 sums, hence the stored bits, do not depend on the machine's core count
    tf = load_reference(Path(a.ref))
    for name, case in CASES.items():
        run_case(tf, name, *case, Path(a.out))


if __name__ == "__main__":
    main()
