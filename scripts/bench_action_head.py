"""Dev measurement (GPU): ActionHead (lipvq-vae_amd/action_head.py) against the plain-torch restatement of the same op sequence
(tests/action_head_ref.py: F.linear, tanh, MSELoss, SmoothL1Loss, CosineSimilarity, the weighted sum -- what the reference's
ICLTransformer issues), same parameters, same GPU, same process.

    python scripts/bench_action_head.py [B ...]     (default: 8 and 4096 -- the ICRT step shape and a large batch; T = 10, E = 512, A = 12)

Per shape: the losses' forward + backward (eager, action_loss with the weights 0.5 / 2.0 / 0.25 so that all three terms run), the
eval-mode forward (eager), and that forward as ONE HIP-graph replay on either side (nnfn.GraphedEval).  feats is the view
``out[:, -T:]`` of a [B, 3T, E] tensor, as the backbone hands it over (the replays take its dense copy).  The two sides ALTERNATE
round by round after a warm-up, the figure is the median of 7 rounds with the rounds' minimum and maximum beside it, and the shader
clock (rocm-smi, read right after the timed windows) is printed beside every line: a time without its clock does not compare
across devices.  Ranges that overlap are "not faster"."""
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
import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd.action_head import ActionHead  # noqa: E402
from lipvq_vae_amd.nnfn import GraphedEval  # noqa: E402

T, E, A = 10, 512, 12
WEIGHTS = (0.5, 2.0, 0.25)
ROUNDS = 7


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
    """tests/action_head_ref.py over the parameters of an ActionHead (shared storage)."""

    def __init__(self, head):
        super().__init__()
        self.head = head

    def losses(self, feats, target, *weights):
        return action_head_ref.head_losses(dict(self.head.named_parameters()), feats, target, weights)

    def forward(self, feats):
        return action_head_ref.actions(dict(self.head.named_parameters()), feats)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fa, fb, n, rounds=ROUNDS):
    for _ in range(10):                                             # warm clock, warm caches, first-use work
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, n))
        tb.append(window(fb, n))
    verdict = "faster" if max(ta) < min(tb) else ("SLOWER" if min(ta) > max(tb) else "not faster (ranges overlap)")
    spread = f"[{min(ta):.4f}-{max(ta):.4f}] / [{min(tb):.4f}-{max(tb):.4f}]"
    return statistics.median(ta), statistics.median(tb), f"{sclk()}   min-max {spread}   ours is {verdict}"


def main():
    batches = [int(a) for a in sys.argv[1:]] or [8, 4096]
    print(f"device {torch.cuda.get_device_name(0)}; T={T} E={E} ac_dim={A} weights={WEIGHTS}; times in ms (ours / plain torch), "
          f"median of {ROUNDS} alternating rounds")
    for B in batches:
        torch.manual_seed(0)
        ours = ActionHead(E, A).cuda()
        ref = TorchHead(ours)
        full = torch.randn(B, 3 * T, E, device="cuda", requires_grad=True)
        target = torch.rand(B, T, A, device="cuda") * 3.0 - 1.5
        n = 1000 if B <= 64 else 50
        ours.train(); ref.train()
        with torch.no_grad():
            lo, lr = (float(m.losses(full[:, -T:], target, *WEIGHTS)["action_loss"]) for m in (ours, ref))

        def step(m):
            ours.zero_grad(set_to_none=True)
            full.grad = None
            m.losses(full[:, -T:], target, *WEIGHTS)["action_loss"].backward()
        t_o, t_r, c = alternate(lambda: step(ours), lambda: step(ref), n)
        print(f"B={B}: losses forward + backward, eager {t_o:9.4f} / {t_r:9.4f}   ratio {t_r / t_o:5.2f}   sclk {c}   "
              f"(rel diff of the loss {abs(lo - lr) / abs(lr):.1e})")
        ours.eval(); ref.eval()
        feats = full.detach()[:, -T:]
        with torch.no_grad():
            t_o, t_r, c = alternate(lambda: ours(feats), lambda: ref(feats), n)
            print(f"B={B}: eval forward, eager               {t_o:9.4f} / {t_r:9.4f}   ratio {t_r / t_o:5.2f}   sclk {c}")
            dense = feats.contiguous()
            g_o, g_r = GraphedEval(ours, dense), GraphedEval(ref, dense)
            t_o, t_r, c = alternate(lambda: g_o(dense), lambda: g_r(dense), n)
            print(f"B={B}: eval forward, one graph replay    {t_o:9.4f} / {t_r:9.4f}   ratio {t_r / t_o:5.2f}   sclk {c}")
        del ours, ref, full, g_o, g_r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
