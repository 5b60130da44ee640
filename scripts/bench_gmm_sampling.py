"""Dev measurement (GPU): GMMActionHead's eval-mode sampling forward under the "kernel" sample source (one dropout_begin launch
and one sampling launch that draws its own noise; include/lipvq.h, "in-kernel sampling") against the "torch" source (torch.rand,
torch.randn and the sampling launch that reads them: the default, unchanged) -- the SAME module, switched between the windows,
same GPU, same process.

    python scripts/bench_gmm_sampling.py [B ...]     (default: 8 and 4096; T = 10, E = 512, M = 5, A = 12)

feats is the view ``out[:, -T:]`` of a [B, 3T, E] tensor, as the backbone hands it over.  Per shape: the eager call, and ONE
nnfn.GraphedEval replay (one capture per source; the captured module reads the view of a tensor it holds, so a replay copies in
one dummy element and the figure is the launches').  The sides take turns window by window after a warm-up; the figure is the
median of 7 windows with their minimum and maximum, and the shader clock (rocm-smi, read right after the last window) is printed
beside every line.  A pair in which the kernel source is slower is marked."""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import torch  # noqa: E402

import lipvq_vae_amd  # noqa: E402,F401
from bench_gmm import A, E, M, T, sclk, window  # noqa: E402
from lipvq_vae_amd.gmm import GMMActionHead  # noqa: E402
from lipvq_vae_amd.nnfn import GraphedEval  # noqa: E402

WINDOWS = 7


class OnView(torch.nn.Module):
    """head on the last T positions of a [B, 3T, E] tensor the module holds: what a GraphedEval capture of the view path replays."""

    def __init__(self, head, full):
        super().__init__()
        self.head, self.full = head, full

    def forward(self, _):
        return self.head(self.full[:, -T:])


def take_turns(f_kernel, f_torch, n):
    for _ in range(3):
        f_kernel(); f_torch()
    torch.cuda.synchronize()
    tk, tt = [], []
    for _ in range(WINDOWS):
        tk.append(window(f_kernel, n))
        tt.append(window(f_torch, n))
    return statistics.median(tk), statistics.median(tt), f"{sclk()}   min-max [{min(tk):.4f}-{max(tk):.4f}] / [{min(tt):.4f}-{max(tt):.4f}]"


def line(B, what, tk, tt, c):
    mark = "" if tk <= tt else "   ** the kernel source is SLOWER **"
    print(f"B={B}: {what} {tk * 1e3:9.1f} / {tt * 1e3:9.1f} us   torch / kernel {tt / tk:5.2f}   sclk {c}{mark}")


def main():
    batches = [int(a) for a in sys.argv[1:]] or [8, 4096]
    print(f"device {torch.cuda.get_device_name(0)}; T={T} E={E} modes={M} ac_dim={A}; eval sampling forward, times in us "
          f"(kernel source / torch source), median of {WINDOWS} alternating windows")
    for B in batches:
        torch.manual_seed(0)
        head = GMMActionHead(E, A, num_modes=M).cuda().eval()
        full = torch.randn(B, 3 * T, E, device="cuda")
        feats = full[:, -T:]
        n = 2000 if B <= 64 else 400                           # 0.05 - 0.15 s per window

        def eager(source):
            def run():
                head.set_sample_source(source)
                head(feats)
            return run
        with torch.no_grad():
            head.set_sample_source("kernel", seed=1)
            tk, tt, c = take_turns(eager("kernel"), eager("torch"), n)
            line(B, "eager            ", tk, tt, c)
            net, dummy = OnView(head, full).eval(), torch.zeros(1, device="cuda")
            graphs = {}
            for source in ("kernel", "torch"):
                head.set_sample_source(source)
                graphs[source] = GraphedEval(net, dummy)
            tk, tt, c = take_turns(lambda: graphs["kernel"](dummy), lambda: graphs["torch"](dummy), n)
            line(B, "one graph replay ", tk, tt, c)
        del head, full, feats, graphs, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
