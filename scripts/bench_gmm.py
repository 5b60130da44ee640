"""Dev measurement (GPU): GMMActionHead (lipvq-vae_amd/gmm.py) against the plain-torch restatement of the same op sequence
(tests/gmm_ref.py: what the reference's decoder + policy_nets.py:2545-2599 issue), same parameters, same GPU, same process.

    python scripts/bench_gmm.py [B ...]          (default: 8 and 4096 -- the ICRT step shape and a large batch; T = 10, E = 512, M = 5, A = 12)

Per shape: the NLL's forward + backward (eager), the eval-mode sampling forward (eager), and that forward as ONE HIP-graph
replay (nnfn.GraphedEval) -- beside the restatement's EAGER ``.sample()``: torch's MixtureSameFamily.sample() cannot be captured
(it fails inside torch.cuda.graph), so there is no torch replay to put beside ours.  feats is the view
``out[:, -T:]`` of a [B, 3T, E] tensor, as the backbone hands it over.  The two sides ALTERNATE round by round after a warm-up,
the figure is the median round with the rounds' minimum and maximum beside it, and the shader clock (rocm-smi, read right after
the timed window) is printed beside every line: a time without its clock does not compare across devices."""
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402

import gmm_ref  # noqa: E402
import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd.gmm import GMMActionHead  # noqa: E402
from lipvq_vae_amd.nnfn import GraphedEval  # noqa: E402

T, E, M, A = 10, 512, 5, 12


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


class TorchHead(torch.nn.Module):
    """tests/gmm_ref.py over the parameters of a GMMActionHead (shared storage)."""

    def __init__(self, head):
        super().__init__()
        self.head = head

    def dist(self, feats, low_noise):
        return gmm_ref.gmm_dist(dict(self.head.named_parameters()), feats, M, A, self.head.min_std, self.head.std_activation, low_noise)

    def nll(self, feats, actions):
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


def main():
    batches = [int(a) for a in sys.argv[1:]] or [8, 4096]
    print(f"device {torch.cuda.get_device_name(0)}; T={T} E={E} modes={M} ac_dim={A}; times in ms (ours / plain torch), median of alternating rounds")
    for B in batches:
        torch.manual_seed(0)
        ours = GMMActionHead(E, A, num_modes=M).cuda()
        ref = TorchHead(ours)
        full = torch.randn(B, 3 * T, E, device="cuda", requires_grad=True)
        actions = torch.rand(B, T, A, device="cuda") * 3.0 - 1.5
        n = 300 if B <= 64 else 20
        ours.train(); ref.train()
        with torch.no_grad():
            d = abs(float(ours.nll(full[:, -T:], actions)) - float(ref.nll(full[:, -T:], actions))) / abs(float(ref.nll(full[:, -T:], actions)))

        def step(m):
            ours.zero_grad(set_to_none=True)
            full.grad = None
            m.nll(full[:, -T:], actions).backward()
        t_o, t_r, c = alternate(lambda: step(ours), lambda: step(ref), n)
        print(f"B={B}: nll forward + backward, eager {t_o:9.3f} / {t_r:9.3f}   ratio {t_r / t_o:5.2f}   sclk {c}   (rel diff of the loss {d:.1e})")
        ours.eval(); ref.eval()
        feats = full.detach()[:, -T:]
        with torch.no_grad():
            t_o, t_r, c = alternate(lambda: ours(feats), lambda: ref(feats), n)
            print(f"B={B}: eval forward (sample), eager  {t_o:9.3f} / {t_r:9.3f}   ratio {t_r / t_o:5.2f}   sclk {c}")
            dense = feats.contiguous()
            g_o = GraphedEval(ours, dense)
            t_o, t_r, c = alternate(lambda: g_o(dense), lambda: ref(dense), n)
            print(f"B={B}: eval forward (sample), our graph replay / torch eager  {t_o:9.3f} / {t_r:9.3f}   ratio {t_r / t_o:5.2f}   sclk {c}")
        del ours, ref, full, g_o
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
