"""Dev measurement (GPU): GPTBackbone (lipvq-vae_amd/gpt.py) against the plain-torch restatement of the same op sequence
(tests/gpt_ref.py: what the reference's eager GPT_Backbone issues), same parameters, same GPU, same process.

    python scripts/bench_gpt.py [B ...]          (default: 8 and 4096 -- the ICRT step shape and a large batch; L = 30, E = 512, 6 layers)

Per shape: the eval forward and a training forward + backward (dropout 0.1: the attention mask drawn by torch.rand and the two
block-output dropouts by F.dropout, on both sides), each eager
and as ONE HIP-graph replay.  The two sides ALTERNATE round by round after a warm-up of every shape, the figure is the median
round with the rounds' minimum and maximum beside it, and the shader clock (rocm-smi, read right after the timed window) is printed beside every line: a time without its
clock does not compare across devices."""
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402

import gpt_ref  # noqa: E402
import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd.gpt import GPTBackbone, GraphedGPTBackbone  # noqa: E402

L, E, H, LAYERS, P = 30, 512, 8, 6, 0.1


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


class TorchBackbone(torch.nn.Module):
    """tests/gpt_ref.py over the parameters of a GPTBackbone (shared storage)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        sd = dict(self.net.named_parameters())
        sd.update(dict(self.net.named_buffers()))
        B = x.shape[0]
        for i in range(LAYERS):
            keeps = None
            if self.training:
                keeps = (torch.rand((B, H, L, L), device=x.device) >= P, None, None)
            x = gpt_ref.block_forward(sd, f"nets.transformer.{i}.nets.", x, H, keeps, (1 - P, 1.0, 1.0), P if self.training else 0.0)
        return torch.nn.functional.layer_norm(x, (E,), sd["nets.output_ln.weight"], sd["nets.output_ln.bias"], 1e-5)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fa, fb, n, rounds=5):
    for _ in range(3):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, n))
        tb.append(window(fb, n))
    spread = f"[{min(ta):.3f}-{max(ta):.3f}] / [{min(tb):.3f}-{max(tb):.3f}]"
    return statistics.median(ta), statistics.median(tb), f"{sclk()}   min-max {spread}"


def graphed_step(module, x):
    """forward + backward of `module` on the static input x as one graph; returns the replay callable."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            module.zero_grad(set_to_none=True)
            module(x).square().mean().backward()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    module.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        module(x).square().mean().backward()
    return graph.replay


def main():
    batches = [int(a) for a in sys.argv[1:]] or [8, 4096]
    print(f"device {torch.cuda.get_device_name(0)}; L={L} E={E} heads={H} layers={LAYERS}; times in ms (ours / plain torch), median of alternating rounds")
    for B in batches:
        torch.manual_seed(0)
        ours = GPTBackbone(E, L).cuda()
        ref = TorchBackbone(ours)
        x = torch.randn(B, L, E, device="cuda")
        n = 300 if B <= 64 else 4
        ours.eval(); ref.eval()
        with torch.no_grad():
            d = ((ours(x) - ref(x)).abs().max() / ref(x).abs().max()).item()
            t_o, t_r, c = alternate(lambda: ours(x), lambda: ref(x), n)
            print(f"B={B}: eval forward, eager        {t_o:9.3f} / {t_r:9.3f}   ratio {t_r / t_o:5.2f}   sclk {c}   (max rel diff {d:.1e})")
            g_o = GraphedGPTBackbone(ours, x)
            gr = torch.cuda.CUDAGraph()
            for _ in range(3):
                ref(x)
            torch.cuda.synchronize()
            with torch.cuda.graph(gr):
                ref(x)
            same = torch.equal(g_o(x), ours(x))
            t_o, t_r, c = alternate(lambda: g_o(x), gr.replay, n)
            print(f"B={B}: eval forward, graph replay {t_o:9.3f} / {t_r:9.3f}   ratio {t_r / t_o:5.2f}   sclk {c}   (replay == eager: {same})")
        ours.train(); ref.train()

        def step(m):
            m.zero_grad(set_to_none=True)
            m(x).square().mean().backward()
        t_o, t_r, c = alternate(lambda: step(ours), lambda: step(ref), max(2, n // 2))
        print(f"B={B}: forward + backward, eager  {t_o:9.3f} / {t_r:9.3f}   ratio {t_r / t_o:5.2f}   sclk {c}")
        r_o, r_r = graphed_step(ours, x), graphed_step(ref, x)
        t_o, t_r, c = alternate(r_o, r_r, max(2, n // 2))
        print(f"B={B}: forward + backward, graph  {t_o:9.3f} / {t_r:9.3f}   ratio {t_r / t_o:5.2f}   sclk {c}")
        del ours, ref, x, r_o, r_r, g_o, gr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
