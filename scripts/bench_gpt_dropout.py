"""Dev measurement (GPU): GPTBackbone's training iteration under its two dropout sources -- "torch" (masks from torch's generator:
torch.rand + compare + cast for the attention bytes, F.dropout on the two branches, per block) against "kernel" (decisions drawn
inside the HIP kernels, lipvq-vae_amd/csrc/lipvq_rng.h) -- same parameters, same GPU, same process.

    python scripts/bench_gpt_dropout.py [B ...]          (default: 8 and 4096 -- the ICRT step shape and a large batch)

Shape: E = 512, 8 heads, 6 layers, L = 30, attn_dropout = block_output_dropout = 0.1 (the ICRT configuration).  Per batch size:
forward + backward, eager; at the first batch size also the whole iteration (zero_grad, backbone, ActionHead loss, backward, Adam
with clipping) as ONE icl.GraphedPolicyStep replay.  The two sides ALTERNATE window by window after a warm-up; the figure is the
median of 7 windows with their minimum and maximum beside it, and the shader clock (rocm-smi, read right after the timed windows)
is printed beside every line: a time without its clock does not compare across devices.  torch.cuda.max_memory_allocated of one
forward + backward is reported for both sources (what the masks and torch's saved tensors cost)."""
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd import optim  # noqa: E402
from lipvq_vae_amd.action_head import ActionHead  # noqa: E402
from lipvq_vae_amd.gpt import GPTBackbone  # noqa: E402
from lipvq_vae_amd.icl import GraphedPolicyStep  # noqa: E402

E, H, LAYERS, L, P, T, A = 512, 8, 6, 30, 0.1, 10, 7
WINDOWS = 7


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


def alternate(fa, fb, n):
    for _ in range(3):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(WINDOWS):
        ta.append(window(fa, n))
        tb.append(window(fb, n))
    spread = f"[{min(ta):.3f}-{max(ta):.3f}] / [{min(tb):.3f}-{max(tb):.3f}]"
    return statistics.median(ta), statistics.median(tb), f"{sclk()}   min-max {spread}"


def backbone(source):
    torch.manual_seed(0)
    net = GPTBackbone(E, L, attn_dropout=P, block_output_dropout=P, num_layers=LAYERS, num_heads=H).cuda().train()
    return net.set_dropout_source(source, seed=1 if source == "kernel" else None)


def peak_mib(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def line(what, t_k, t_t, c):
    slower = "   **kernel source slower**" if t_k > t_t else ""
    print(f"{what}: kernel {t_k:9.3f} / torch {t_t:9.3f}   torch / kernel {t_t / t_k:5.2f}   sclk {c}{slower}", flush=True)


def main():
    batches = [int(a) for a in sys.argv[1:]] or [8, 4096]
    print(f"device {torch.cuda.get_device_name(0)}; E={E} heads={H} layers={LAYERS} L={L} p={P}; times in ms, median of {WINDOWS} "
          f"alternating windows", flush=True)
    for k, B in enumerate(batches):
        nets = {s: backbone(s) for s in ("kernel", "torch")}
        x = torch.randn(B, L, E, device="cuda", requires_grad=True)
        n = 30 if B <= 64 else 3

        def step(net):
            net.zero_grad(set_to_none=True)
            x.grad = None
            net(x).square().mean().backward()
        t_k, t_t, c = alternate(lambda: step(nets["kernel"]), lambda: step(nets["torch"]), n)
        line(f"B={B}: forward + backward, eager", t_k, t_t, c)
        m_k, m_t = peak_mib(lambda: step(nets["kernel"])), peak_mib(lambda: step(nets["torch"]))
        print(f"B={B}: peak memory of one forward + backward above the resident tensors: kernel {m_k:9.1f} MiB / torch {m_t:9.1f} MiB "
              f"(torch - kernel = {m_t - m_k:.1f} MiB)", flush=True)
        if k == 0:
            steps = {}
            for s, net in nets.items():
                torch.manual_seed(1)
                head = ActionHead(E, A).cuda().train()
                params = list(net.parameters()) + list(head.parameters())
                opt = optim.Adam(params, lr=torch.tensor(1e-4, device="cuda"), max_grad_norm=1.0)
                target = torch.rand(B, T, A, device="cuda") * 2.0 - 1.0
                loss_fn = lambda xx, aa, net=net, head=head: head.losses(net(xx)[:, -T:], aa)["action_loss"]      # noqa: E731
                extra = [net.dropout_state] if s == "kernel" else []
                g = GraphedPolicyStep(loss_fn, params, opt, (x.detach(), target), extra_state=extra)
                steps[s] = (g, x.detach(), target)
            t_k, t_t, c = alternate(lambda: steps["kernel"][0].step(*steps["kernel"][1:]), lambda: steps["torch"][0].step(*steps["torch"][1:]), 50)
            line(f"B={B}: whole iteration, GraphedPolicyStep replay", t_k, t_t, c)
            params = [p for p in nets["kernel"].parameters()]
            assert all(bool(torch.isfinite(p).all()) for p in params), "the replayed steps left a parameter that is not finite"
            del steps
        del nets, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
