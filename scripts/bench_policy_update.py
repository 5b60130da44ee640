"""Dev measurement (GPU): the policy's update -- clip, gradient-norm report, Adam -- at the ICRT policy's parameter list
(GPTBackbone(512, 30), 6 layers, 8 heads, plus GMMActionHead(512, 12, 5 modes)), the gradients already present.

    python scripts/bench_policy_update.py [--rounds R] [--n N]

Sides, each on parameters, gradients and optimizer state of its own, taking turns round by round in one process after a
warm-up of all of them (median round, minimum and maximum beside it, the shader clock read right after the timed windows):

  (a) the reference's sequence (robomimic/utils/torch_utils.py:196-234): torch.nn.utils.clip_grad_norm_, the loop of
      p.grad.norm(2).pow(2).item() -- one host synchronisation per parameter --, torch.optim.Adam.step(), with Adam in its default
      form and as Adam(capturable=True, foreach=True);
  (b) ours: optim.Adam(max_grad_norm=1.0).step() followed by the one .item() of backprop_for_loss, the same without the .item(),
      and the step as a HIP-graph replay.

Each figure is a host clock around N iterations that end in a device synchronise: what a training loop waits for.  Last, the
sum-of-squares launches alone (device events around N repetitions): the gradient bytes they read over the time."""
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd import _capi, ops, optim  # noqa: E402
from lipvq_vae_amd.gmm import GMMActionHead  # noqa: E402
from lipvq_vae_amd.gpt import GPTBackbone  # noqa: E402

MAX_NORM = 1.0


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


def policy_parameters(seed):
    """Fresh parameters of the ICRT policy's list with a gradient on each (norm well above MAX_NORM: the clip binds)."""
    torch.manual_seed(0)
    net = torch.nn.ModuleList([GPTBackbone(512, 30, num_layers=6, num_heads=8), GMMActionHead(512, 12, num_modes=5)]).cuda()
    ps = list(net.parameters())
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2
    return ps


def reference_sequence(ps, opt):
    def run():
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        grad_norms = 0.0
        for p in ps:
            if p.grad is not None:
                grad_norms += p.grad.data.norm(2).pow(2).item()
        opt.step()
        return grad_norms
    return run


def wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    args = sys.argv[1:]
    opt_int = lambda name, default: int(args[args.index(name) + 1]) if name in args else default
    rounds, n = opt_int("--rounds", 7), opt_int("--n", 50)
    sides = []

    ps = policy_parameters(1)
    sides.append(("(a) reference, Adam default", reference_sequence(ps, torch.optim.Adam(ps, lr=1e-4, weight_decay=1e-4))))
    ps = policy_parameters(1)
    sides.append(("(a) reference, Adam capturable foreach",
                  reference_sequence(ps, torch.optim.Adam(ps, lr=1e-4, weight_decay=1e-4, capturable=True, foreach=True))))
    ps = policy_parameters(1)
    ours = optim.Adam(ps, lr=torch.tensor(1e-4, device="cuda"), weight_decay=1e-4, max_grad_norm=MAX_NORM)
    sides.append(("(b) ours eager + one .item()", lambda: (ours.step(), ours.grad_stats[3].item())))
    ps = policy_parameters(1)
    ours_nosync = optim.Adam(ps, lr=torch.tensor(1e-4, device="cuda"), weight_decay=1e-4, max_grad_norm=MAX_NORM)
    sides.append(("(b) ours eager, no synchronisation", ours_nosync.step))
    ps = policy_parameters(1)
    numel, tensors = sum(p.numel() for p in ps), len(ps)
    graphed = optim.Adam(ps, lr=torch.tensor(1e-4, device="cuda"), weight_decay=1e-4, max_grad_norm=MAX_NORM)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            graphed.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    sides.append(("(b) ours, HIP-graph replay", graph.replay))

    print(f"device {torch.cuda.get_device_name(0)}; {tensors} tensors, {numel} parameters; max_norm {MAX_NORM}; "
          f"ms per update, median of {rounds} alternating rounds of {n}")
    for _, f in sides:
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    t = [[] for _ in sides]
    for _ in range(rounds):
        for i, (_, f) in enumerate(sides):
            t[i].append(wall(f, n))
    clock = sclk()
    result = {"tensors": tensors, "parameters": numel, "sclk": clock}
    for (name, _), v in zip(sides, t):
        print(f"{name:<40s} {statistics.median(v):8.3f}   [{min(v):.3f}-{max(v):.3f}]   sclk {clock}")
        result[name] = round(statistics.median(v), 4)

    # the sum-of-squares launches alone
    grads = [p.grad for p in ps]
    ws = torch.empty(_capi.lib.lipvq_grad_sumsq_workspace_bytes(tensors) // 8, dtype=torch.float64, device="cuda")
    calls = []
    for s in range(0, tensors, 32):
        chunk = grads[s:s + 32]
        calls.append(((C.c_void_p * len(chunk))(*[g.data_ptr() for g in chunk]), (C.c_int64 * len(chunk))(*[g.numel() for g in chunk]),
                      len(chunk), s))

    def sumsq():
        st = ops._stream()
        for ptrs, numels, count, first in calls:
            _capi.check(_capi.lib.lipvq_grad_sumsq_f32(ptrs, numels, count, first, tensors, ws.data_ptr(), st), "lipvq_grad_sumsq_f32")

    for _ in range(10):
        sumsq()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(200):
            sumsq()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 200)
    ms = statistics.median(times)
    print(f"sum of squares alone ({len(calls)} launches): {ms * 1e3:.1f} us for {4 * numel / 1e6:.1f} MB of gradients = "
          f"{4 * numel / (ms * 1e-3) / 1e12:.2f} TB/s   [{min(times) * 1e3:.1f}-{max(times) * 1e3:.1f} us]   sclk {sclk()}")
    result["sumsq_us"], result["sumsq_TBps"] = round(ms * 1e3, 2), round(4 * numel / (ms * 1e-3) / 1e12, 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
