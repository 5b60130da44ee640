"""Dev measurement (GPU): the three matmul precisions of the output heads (ActionHead / GMMActionHead.set_matmul_precision: "fp32",
"bf16", "bf16x3") and the plain-torch restatement of the same op sequence (tests/action_head_ref.py, tests/gmm_ref.py), same
parameters, same GPU, same process.

    python scripts/bench_head_precision.py [B ...]     (default: 8 and 4096 -- the ICRT step shape and a large batch;
                                                        T = 10, E = 512, A = 12, M = 5)

Per head and shape: the eval forward (eager), that forward as ONE HIP-graph replay (nnfn.GraphedEval), and the loss forward +
backward (eager: ActionHead's action_loss with the weights 0.5 / 2.0 / 0.25, the GMM head's NLL).  feats is the view
``out[:, -T:]`` of a [B, 3T, E] tensor, as the backbone hands it over (the replays take its dense copy).  torch's
MixtureSameFamily.sample() cannot be captured, so the GMM head's replay line has no torch side.  The four sides take turns, window by
window, after a warm-up; a figure is the median of 7 windows with their minimum and maximum beside it, and the shader clock
(rocm-smi, read right after the timed windows) is printed with every line: a time without its clock does not compare across
devices.  Two sides whose ranges overlap are "not separated".  Output: one markdown table row per line."""
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402

import action_head_ref  # noqa: E402
import gmm_ref  # noqa: E402
import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd.action_head import ActionHead  # noqa: E402
from lipvq_vae_amd.gmm import GMMActionHead  # noqa: E402
from lipvq_vae_amd.nnfn import GraphedEval  # noqa: E402

T, E, A, M = 10, 512, 12, 5
WEIGHTS = (0.5, 2.0, 0.25)
ROUNDS = 7
SIDES = ("fp32", "bf16", "bf16x3", "torch")


def sclk():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=10)
        for card in json.loads(r.stdout).values():
            for k, v in card.items():
                if k.lower().startswith("sclk clock speed"):
                    return str(v).strip("()Mhz ") + " MHz"
    except Exception:
        pass
    return "n/a"


class TorchAction(torch.nn.Module):
    """tests/action_head_ref.py over the parameters of an ActionHead (shared storage)."""

    def __init__(self, head):
        super().__init__()
        self.head = head

    def loss(self, feats, target):
        return action_head_ref.head_losses(dict(self.head.named_parameters()), feats, target, WEIGHTS)["action_loss"]

    def forward(self, feats):
        return action_head_ref.actions(dict(self.head.named_parameters()), feats)


class TorchGmm(torch.nn.Module):
    """tests/gmm_ref.py over the parameters of a GMMActionHead (shared storage)."""

    def __init__(self, head):
        super().__init__()
        self.head = head

    def dist(self, feats, low_noise):
        return gmm_ref.gmm_dist(dict(self.head.named_parameters()), feats, M, A, self.head.min_std, self.head.std_activation, low_noise)

    def loss(self, feats, actions):
        return -self.dist(feats, False).log_prob(actions).mean()

    def forward(self, feats):
        return self.dist(feats, self.head.low_noise_eval and not self.training).sample()


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def take_turns(fns, n, rounds=ROUNDS):
    """fns: {side: callable or None}.  {side: (median, min, max)} in ms, and the shader clock after the last window."""
    live = {k: f for k, f in fns.items() if f is not None}
    for _ in range(10):                                             # warm clock, warm caches, first-use work
        for f in live.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in live}
    for _ in range(rounds):
        for k, f in live.items():
            times[k].append(window(f, n))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}, sclk()


def row(head, B, what, res, clock):
    cells = []
    for k in SIDES:
        cells.append("n/a" if k not in res else f"{res[k][0]:.4f} [{res[k][1]:.4f}-{res[k][2]:.4f}]")
    notes = []
    for k in ("bf16", "bf16x3"):
        for other in ("fp32", "torch"):
            if other in res:
                v = "faster than" if res[k][2] < res[other][1] else ("SLOWER than" if res[k][1] > res[other][2] else "not separated from")
                notes.append(f"{k} {v} {other}")
    print(f"| {head} | {B} | {what} | " + " | ".join(cells) + f" | {clock} | " + "; ".join(notes) + " |", flush=True)


def make_sides(cls, torch_cls, *args):
    """One module per precision and the torch restatement, all over the SAME parameter values."""
    torch.manual_seed(0)
    base = cls(*args).cuda()
    sides = {}
    for p in SIDES[:3]:
        m = cls(*args).cuda().set_matmul_precision(p)
        m.load_state_dict(base.state_dict())
        sides[p] = m
    sides["torch"] = torch_cls(base)
    return sides


def bench(name, sides, B, loss_of, graph_torch):
    full = torch.randn(B, 3 * T, E, device="cuda", requires_grad=True)
    target = torch.rand(B, T, A, device="cuda") * 2.0 - 1.0
    n = 500 if B <= 64 else 30
    for m in sides.values():
        m.eval()
    feats = full.detach()[:, -T:]
    dense = feats.contiguous()
    with torch.no_grad():
        res, clock = take_turns({k: (lambda m=m: m(feats)) for k, m in sides.items()}, n)
        row(name, B, "eval forward, eager", res, clock)
        graphs = {k: (GraphedEval(m, dense) if (k != "torch" or graph_torch) else None) for k, m in sides.items()}
        res, clock = take_turns({k: (None if g is None else (lambda g=g: g(dense))) for k, g in graphs.items()}, n)
        row(name, B, "eval forward, one graph replay", res, clock)
    for m in sides.values():
        m.train()

    def step(m):
        for s in sides.values():
            s.zero_grad(set_to_none=True)
        full.grad = None
        loss_of(m, full[:, -T:], target).backward()
    res, clock = take_turns({k: (lambda m=m: step(m)) for k, m in sides.items()}, n)
    row(name, B, "loss forward + backward, eager", res, clock)
    with torch.no_grad():
        losses = {k: float(loss_of(m, full[:, -T:], target)) for k, m in sides.items()}
    print(f"    ({name} B={B}: loss " + ", ".join(f"{k} {v:.7f}" for k, v in losses.items()) + ")", flush=True)


def main():
    batches = [int(a) for a in sys.argv[1:]] or [8, 4096]
    print(f"device {torch.cuda.get_device_name(0)}; T={T} E={E} ac_dim={A} num_modes={M}; ms per call, median of {ROUNDS} windows taking "
          f"turns [min-max]")
    print("| head | B | what | " + " | ".join(SIDES) + " | sclk | ranges |")
    print("|---|---|---|---|---|---|---|---|---|")
    for B in batches:
        bench("ActionHead", make_sides(ActionHead, TorchAction, E, A), B, lambda m, f, t: (
            m.loss(f, t) if isinstance(m, TorchAction) else m.losses(f, t, *WEIGHTS)["action_loss"]), True)
        bench("GMMActionHead", make_sides(GMMActionHead, TorchGmm, E, A, M), B, lambda m, f, t: (
            m.loss(f, t) if isinstance(m, TorchGmm) else m.nll(f, t)), False)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
