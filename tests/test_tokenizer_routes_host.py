"""Which launches a tokenizer call runs ("Which launches a call runs"), pinned on the host.

The launching functions of ``lipvq_vae_amd.ops`` are replaced with recorders that return CPU tensors of the right shapes and
dtypes; the pure host queries (``tokenize_supported``, ``nearest_screen_supported``, ``mlp3_loss_supported`` ...) stay real, and
the module's screen monitor is replaced with one whose answer the case sets.  Each case runs one entry point TWICE on a fresh
module (the second call pins what the pack / prepare / workspace caches skip) and yields, per call, the ordered list of launches
with every argument that selects behaviour (activation triple, distance rule, save_pre / want_pre / want_ze, which optional
operands were passed, loss weight and form, row counts: tensors are recorded as their shapes) and the number of times the monitor
was consulted.

``tests/golden/tokenizer_routes.json`` holds those lists as recorded from the commit BEFORE the routing policy was gathered into
``_TokenizerBase._plan``: the test asserts that today's code issues the same launches, in order and in arguments, and consults
the monitor as often (with the one exception listed under ``FEWER_CONSULTATIONS``).  To record from another checkout
(its library: ``LIPVQ_HIP_LIBRARY``, see ``_capi.py``):

    LIPVQ_HIP_LIBRARY=<a build of the same csrc> python tests/test_tokenizer_routes_host.py <checkout root> [out.json]
"""
import inspect
import json
import sys
from pathlib import Path

import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "tokenizer_routes.json"

LAUNCHERS = ("lipschitz_scale", "mlp3_pack", "mlp3_pack_f16", "mlp3", "mlp3_loss", "mse_pair_loss", "ste",
             "nearest", "nearest_rows", "nearest_prepare", "nearest_screened", "tokenize_workspace", "tokenize", "vq_tokenize",
             "scaled_diff", "mlp3_pack_bwd2", "mlp3_bwd", "wgrad", "scatter_add_vq", "lipschitz_bwd")

# name -> (class, constructor arguments)
MODELS = {
    "llfq_d64_k1024": ("LLFQVAE_V4", (7, 64, 1024), {}),                         # the fused shape
    "llfq_d48_k1024": ("LLFQVAE_V4", (7, 48, 1024), {}),                         # screened, not fused
    "llfq_d64_k1024_h64": ("LLFQVAE_V4", (7, 64, 1024), {"hidden_dim": 64}),     # not fused
    "llfq_d520_k256": ("LLFQVAE_V4", (7, 520, 256), {}),                         # wider than any screen
    "vq_d64_k32": ("VQVAE", (7, 64), {"num_embeddings": 32}),
    "vq_d64_k128": ("VQVAE", (7, 64), {"num_embeddings": 128}),
    "vq_d64_k512": ("VQVAE", (7, 64), {"num_embeddings": 512}),
    "vq_d48_k512": ("VQVAE", (7, 48), {"num_embeddings": 512}),
}
# both sides of EXACT_ROWS_MAX and of the folded decoder's 65 536-row rule
ROWS = (0, 1, 2048, 2049, 65535, 65536, 70000)
ENTRIES = ("tokenize", "tokenize_no_usage", "tokenize_fast", "forward_no_grad", "forward_loss_backward", "forward_backward")

# Cases that may consult the monitor FEWER times than the fixture.  Reason: at a latent width above 512 there is no screened route at
# all (no fused launch, no stand-alone screen), so the answer cannot change anything; the recorded code asked anyway for every batch
# above EXACT_ROWS_MAX, the plan asks only where a screened route exists.  (tokenize_fast raises before any routing there.)
FEWER_CONSULTATIONS = {f"llfq_d520_k256/N={n}/monitor={m}/{e}" for n in (2049, 65535, 65536, 70000) for m in (0, 1)
                       for e in ("tokenize", "tokenize_no_usage", "forward_no_grad", "forward_loss_backward", "forward_backward")}


def _summary(v):
    """A launch argument as data: tensors by shape, packed operands by their dimensions, scalars by value."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, torch.Tensor):
        return "T" + "x".join(str(s) for s in v.shape)
    if isinstance(v, (tuple, list)):
        return [_summary(e) for e in v]
    if isinstance(v, torch.device):
        return str(v)
    slots = getattr(type(v), "__slots__", None)                  # PackedMlp3, PreparedCodebook
    if slots:
        return type(v).__name__ + "(" + ",".join(str(getattr(v, s)) for s in slots if s != "buf") + ")"
    return type(v).__name__


class _Monitor:
    """Stand-in for tokenizer._ScreenMonitor: the case's answer, a count of the consultations, record() as a log entry."""

    def __init__(self, answer, log):
        self.answer, self.log, self.asked = answer, log, 0

    def use_screen(self):
        self.asked += 1
        return self.answer

    def record(self, ws, n, coarse=False):
        self.log.append(f"monitor.record(n={int(n)}, coarse={bool(coarse)})")


def _f(*shape):
    return torch.empty(shape, dtype=torch.float32)


def _stubs(ops):
    """name -> function returning what the real launcher returns, as CPU tensors of the right shapes and dtypes."""
    def rows(x, gather_idx=None):
        return x.shape[0] if gather_idx is None else gather_idx.numel()

    def pre3(N, p, save_pre):
        return [_f(N, J) if save_pre else None for J in (p.J0, p.J1, p.J2)]

    def mlp3_pack(W0, b0, W1, b1, W2, b2):
        return ops.PackedMlp3(_f(1), W0.shape[1], W0.shape[0], W1.shape[0], W2.shape[0])

    def mlp3(x, packed, acts, gather_idx=None, N=None, save_pre=False):
        N = rows(x, gather_idx)
        y = _f(N, packed.J2)
        return (y, pre3(N, packed, True)) if save_pre else y

    def mlp3_loss(x, packed, acts, gather_idx, target, latent, w, form, save_pre=False, ste=False):
        N = rows(x, gather_idx)
        out = (_f(N, packed.J2), pre3(N, packed, True) if save_pre else None, _f(3))
        return out + (_f(N, packed.K0),) if ste else out

    def nearest(z, codebook, dist=0, usage=None, want_zq=True, want_best=False):
        N = z.shape[0]
        return torch.zeros(N, dtype=torch.int64), torch.empty_like(z) if want_zq else None, _f(N) if want_best else None

    def nearest_rows(z, codebook, usage=None, want_zq=True, dist=0, route=None):
        return torch.zeros(z.shape[0], dtype=torch.int64), torch.empty_like(z) if want_zq else None

    def nearest_screened(z, codebook, prep, usage=None, want_zq=True, return_workspace=False, debug_gamma=None, dist=0):
        out = (torch.zeros(z.shape[0], dtype=torch.int64), torch.empty_like(z) if want_zq else None)
        return out + (torch.zeros(16, dtype=torch.int32),) if return_workspace else out

    def tokenize(x, packed, raw, codebook, prep, usage=None, want_zq=True, want_ze=False, workspace=None, packed16=None,
                 want_pre=False):
        N, D = x.shape[0], codebook.shape[1]
        out = (torch.zeros(N, dtype=torch.int64), _f(N, D) if want_zq else None, _f(N, D) if (want_ze or want_pre) else None,
               workspace if workspace is not None else torch.zeros(16, dtype=torch.int32))
        return out + (tuple(_f(N, J) for J in (packed.J0, packed.J1, D)),) if want_pre else out

    def vq_tokenize(x, packed, codebook, prep, usage=None, workspace=None, want_pre=False):
        N, D = x.shape[0], codebook.shape[1]
        ws = workspace if workspace is not None else torch.zeros(16, dtype=torch.int32)
        out = (torch.zeros(N, dtype=torch.int64), _f(N, D), _f(N, D))
        return out + ([_f(N, J) for J in (packed.J0, packed.J1, D)], ws) if want_pre else out + (ws,)

    def mlp3_pack_bwd2(a, b):
        return tuple(ops.PackedMlp3(_f(1), W0.shape[1], W0.shape[0], W1.shape[0], W2.shape[0]) for W0, W1, W2 in (a, b))

    def mlp3_bwd(gy, pre, packed_bwd, acts, want_gx=True, in_term=None, out_term=None, gscale=None):
        N, p = pre[0].shape[0], packed_bwd
        return _f(N, p.J2), _f(N, p.J1), _f(N, p.J0), _f(N, p.K0) if want_gx else None

    return {
        "lipschitz_scale": lambda W, ci: (_f(W.shape[0]), torch.empty_like(W)),
        "mlp3_pack": mlp3_pack,
        "mlp3_pack_f16": lambda W0, W1, W2: torch.empty(16, dtype=torch.uint8),
        "mlp3": mlp3,
        "mlp3_loss": mlp3_loss,
        "mse_pair_loss": lambda xr, x, zq, ze, w, form: _f(3),
        "ste": lambda ze, zq: torch.empty_like(ze),
        "nearest": nearest,
        "nearest_rows": nearest_rows,
        "nearest_prepare": lambda codebook: ops.PreparedCodebook(torch.empty(16, dtype=torch.uint8), *codebook.shape),
        "nearest_screened": nearest_screened,
        "tokenize_workspace": lambda N, D, device: torch.zeros(16, dtype=torch.int32),
        "tokenize": tokenize,
        "vq_tokenize": vq_tokenize,
        "scaled_diff": lambda a, b, alpha, gscale=None, c=None: torch.empty_like(a),
        "mlp3_pack_bwd2": mlp3_pack_bwd2,
        "mlp3_bwd": mlp3_bwd,
        "wgrad": lambda G, H, h_act=0, hidx=None, want_bias=True: (_f(G.shape[1], H.shape[1]), _f(G.shape[1]) if want_bias else None),
        "scatter_add_vq": lambda g, ze, table, idx, alpha, gscale=None, zq=None, deterministic=None: torch.empty_like(table),
        "lipschitz_bwd": lambda W, ci, gWn: (torch.empty_like(W), torch.empty_like(ci)),
    }


class _Recorder:
    """Installs the stubs on the ops module; every stubbed call appends `name(argument=summary, ...)` to self.log."""

    def __init__(self, ops):
        self.ops, self.log, self.saved = ops, [], {}
        for name, stub in _stubs(ops).items():
            real = getattr(ops, name)
            self.saved[name] = real
            setattr(ops, name, self._wrap(name, inspect.signature(real), stub))
        assert set(self.saved) == set(LAUNCHERS)

    def _wrap(self, name, sig, stub):
        def call(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            self.log.append(name + "(" + ", ".join(f"{k}={_summary(v)}" for k, v in b.arguments.items()) + ")")
            return stub(*a, **kw)
        return call

    def restore(self):
        for name, real in self.saved.items():
            setattr(self.ops, name, real)


def _entry(pkg, model, entry, x):
    if entry == "tokenize":
        model.tokenize(x)
    elif entry == "tokenize_no_usage":
        model.tokenize(x, count_usage=False)
    elif entry == "tokenize_fast":
        model.tokenize(x, count_usage=False, mode="fast")
    elif entry == "forward_no_grad":
        with torch.no_grad():
            model(x)
    elif entry == "forward_loss_backward":
        model(x)[1].backward()
    else:
        pkg.autograd.forward_backward(model, x)


def record_model(pkg, name):
    """{case name: [[launches of call 1, consultations], [launches of call 2, consultations]]} for one entry of MODELS."""
    import lipvq_vae_amd.autograd  # noqa: F401  (pkg.autograd)
    cls, args, kwargs = MODELS[name]
    rec = _Recorder(pkg.ops)
    out = {}
    try:
        for n in ROWS:
            for answer in (False, True):
                for entry in ENTRIES:
                    if entry == "tokenize_fast" and cls != "LLFQVAE_V4":
                        continue
                    model = getattr(pkg.tokenizer, cls)(*args, **kwargs)
                    mon = model._screen_monitor = _Monitor(answer, rec.log)
                    x = torch.zeros(n, 7)
                    calls = []
                    for _ in range(2):
                        del rec.log[:]
                        mon.asked = 0
                        try:
                            _entry(pkg, model, entry, x)
                        except Exception as e:  # noqa: BLE001 -- what a call raises is part of what it does
                            rec.log.append("raises " + type(e).__name__)
                        calls.append([list(rec.log), mon.asked])
                    out[f"{name}/N={n}/monitor={int(answer)}/{entry}"] = calls
    finally:
        rec.restore()
    return out


def _package():
    import lipvq_vae_amd
    import lipvq_vae_amd.tokenizer  # noqa: F401
    return lipvq_vae_amd


@pytest.fixture(scope="module")
def golden():
    g = json.loads(GOLDEN.read_text())
    # stored compactly: every distinct launch and every distinct sequence of launches once, referred to by position
    seqs = [[g["launches"][i] for i in s] for s in g["sequences"]]
    return {case: [[seqs[s], asked] for s, asked in calls] for case, calls in g["cases"].items()}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_launch_sequences_equal_the_recorded_ones(name, golden):
    got = record_model(_package(), name)
    want = {c: v for c, v in golden.items() if c.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    fewer = set()
    for case in sorted(got):
        for call, ((launches, asked), (launches0, asked0)) in enumerate(zip(got[case], want[case])):
            assert launches == launches0, f"{case}, call {call + 1}: launches differ from the recorded ones"
            assert asked <= 1, f"{case}, call {call + 1}: the monitor was consulted {asked} times in one call"
            if asked < asked0:
                fewer.add(case)
            else:
                assert asked == asked0, f"{case}, call {call + 1}: monitor consulted {asked} times, recorded {asked0}"
    assert fewer == {c for c in FEWER_CONSULTATIONS if c.startswith(name + "/")}


def test_grid_is_the_recorded_grid(golden):
    entries = lambda m: [e for e in ENTRIES if e != "tokenize_fast" or MODELS[m][0] == "LLFQVAE_V4"]  # noqa: E731
    assert sorted(golden) == sorted(f"{m}/N={n}/monitor={a}/{e}" for m in MODELS for n in ROWS for a in (0, 1) for e in entries(m))
    assert FEWER_CONSULTATIONS <= set(golden)


if __name__ == "__main__":
    root = Path(sys.argv[1]).resolve()
    sys.path.insert(0, str(root))
    pkg = _package()
    assert Path(pkg.__file__).resolve().is_relative_to(root), pkg.__file__
    cases = {}
    for m in sorted(MODELS):
        cases.update(record_model(pkg, m))
    launches, sequences = {}, {}
    for calls in cases.values():
        for c in calls:
            seq = tuple(launches.setdefault(line, len(launches)) for line in c[0])
            c[0] = sequences.setdefault(seq, len(sequences))
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN
    out.write_text(json.dumps({"recorded_from": "the commit before _TokenizerBase._plan", "launches": list(launches),
                               "sequences": [list(s) for s in sequences], "cases": cases}, separators=(",", ":")) + "\n")
    print(f"{len(cases)} cases, {len(sequences)} distinct launch sequences -> {out}")
