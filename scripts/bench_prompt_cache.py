"""Dev measurement (GPU): a rollout step of GPTBackbone with the prompt cached (prefill once, forward_cached on the Lq new rows)
against the unchanged full forward on all P + Lq rows -- same module, same parameters, same GPU, same process.

    python scripts/bench_prompt_cache.py [--rounds R] [B ...]     (default B: 1 8 256 4096; E = 512, 8 heads, 6 layers, P = 20, Lq = 10)

Per batch and per matmul precision (fp32, bf16): the eager call and ONE HIP-graph replay of each side.  After a warm-up of every
callable the two sides ALTERNATE window by window; the figure is the median window, the windows' minimum and maximum stand
beside it, and the shader clock (rocm-smi, read right after the timed windows) is printed on every line: a time without its
clock does not compare across devices.  "faster beyond the spread" = the cached side's slowest window beats the full side's
fastest.  prefill is timed separately, once per batch and precision.  Before anything is timed the cached rows are compared
with the full forward's (torch.equal).  The last line is one JSON object with every figure."""
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd.gpt import GPTBackbone, GraphedGPTBackbone, PromptedGPTBackbone  # noqa: E402
from lipvq_vae_amd.nnfn import GraphedEval  # noqa: E402

E, H, LAYERS, P, LQ = 512, 8, 6, 20, 10


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


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fns, n, rounds):
    """Per side: the windows (ms per call) of `rounds` rounds in which the sides take turns, after a warm-up of every side."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            t[i].append(window(f, n))
    return t


def calls_per_window(fn, target_ms=60.0):
    """Enough calls for a window of about target_ms."""
    fn()
    torch.cuda.synchronize()
    one = max(window(fn, 3), 1e-3)
    return max(3, min(2000, int(target_ms / one)))


def main():
    args = sys.argv[1:]
    rounds = 7
    if "--rounds" in args:
        i = args.index("--rounds")
        rounds = int(args[i + 1])
        del args[i:i + 2]
    batches = [int(a) for a in args] or [1, 8, 256, 4096]
    if not torch.cuda.is_available():
        sys.exit("bench_prompt_cache.py measures on the GPU only")
    print(f"device {torch.cuda.get_device_name(0)}; E={E} heads={H} layers={LAYERS} P={P} Lq={LQ}; ms per call, full / cached, "
          f"median of {rounds} alternating windows [min-max]")
    results = []
    torch.manual_seed(0)
    net = GPTBackbone(E, P + LQ).cuda().eval()
    for B in batches:
        x = torch.randn(B, P + LQ, E, device="cuda")
        prompt, new = x[:, :P].contiguous(), x[:, P:].contiguous()
        for prec in ("fp32", "bf16"):
            net.set_matmul_precision(prec)
            with torch.no_grad():
                full = net(x)
                cache = net.prefill(prompt)
                same = torch.equal(net.forward_cached(new, cache), full[:, P:])
                rel = float((net.forward_cached(new, cache) - full[:, P:]).abs().max() / full.abs().max())
                sides = {"eager": [lambda: net(x), lambda: net.forward_cached(new, cache)]}
                g_full = GraphedGPTBackbone(net, x)
                g_cached = GraphedEval(PromptedGPTBackbone(net, cache), new)
                assert torch.equal(g_full(x), full) and torch.equal(g_cached(new), net.forward_cached(new, cache))
                sides["graph"] = [lambda: g_full(x), lambda: g_cached(new)]
                for how, fns in sides.items():
                    n = calls_per_window(fns[0])
                    t = alternate(fns, n, rounds)
                    med = [statistics.median(v) for v in t]
                    beyond = max(t[1]) < min(t[0])
                    print(f"B={B:5d} {prec} {how:5s}: {med[0]:9.4f} [{min(t[0]):.4f}-{max(t[0]):.4f}] / {med[1]:9.4f} "
                          f"[{min(t[1]):.4f}-{max(t[1]):.4f}]   cached / full = {med[1] / med[0]:.3f}   faster beyond the spread: "
                          f"{beyond}   ({n} calls per window, sclk {sclk()})")
                    results.append(dict(B=B, precision=prec, how=how, full_ms=med[0], cached_ms=med[1], full_minmax=[min(t[0]), max(t[0])],
                                        cached_minmax=[min(t[1]), max(t[1])], ratio=med[1] / med[0], faster_beyond_spread=beyond,
                                        calls_per_window=n, bits_equal=same, max_rel_diff=rel))
                n = calls_per_window(lambda: net.prefill(prompt))
                tp = alternate([lambda: net.prefill(prompt)], n, rounds)[0]
                print(f"B={B:5d} {prec} prefill (eager, once per prompt): {statistics.median(tp):9.4f} [{min(tp):.4f}-{max(tp):.4f}]   "
                      f"cache {cache.nbytes / 1024:.0f} KiB   cached rows == full forward's: {same} (max rel diff {rel:.1e})")
                results.append(dict(B=B, precision=prec, how="prefill", ms=statistics.median(tp), minmax=[min(tp), max(tp)],
                                    cache_bytes=cache.nbytes))
                del g_full, g_cached, cache, full, sides
        del x, prompt, new
        torch.cuda.empty_cache()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), E=E, H=H, layers=LAYERS, P=P, Lq=LQ, rounds=rounds, results=results)))


if __name__ == "__main__":
    main()
