"""Dev measurement (GPU): GPTBackbone (lipvq-vae_amd/gpt.py) against the plain-torch restatement of the same op sequence
(tests/gpt_ref.py: what the reference's eager GPT_Backbone issues), same parameters, same GPU, same process.

    python scripts/bench_gpt.py [--precision bf16|bf16x3] [B ...]   (default: 8 and 4096 -- the ICRT step shape and a large
                                                                     batch; L = 30, E = 512, 6 layers)

--precision bf16 measures four sides instead of two: ours with set_matmul_precision("bf16"), ours in fp32 (the same build, the
fp32 kernels), plain torch in fp32 and plain torch under torch.autocast(dtype=torch.bfloat16).
--precision bf16x3 measures ours with set_matmul_precision("bf16x3"), ours in fp32, ours in "bf16" and plain torch in fp32, in
seven alternating rounds instead of five.

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


ROUNDS = 5


def alternate(fns, n, rounds=None):
    """Median per side of `rounds` rounds in which the sides take turns; also the clock and every side's min-max."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds or ROUNDS):
        for i, f in enumerate(fns):
            t[i].append(window(f, n))
    spread = " / ".join(f"[{min(v):.3f}-{max(v):.3f}]" for v in t)
    return [statistics.median(v) for v in t], f"{sclk()}   min-max {spread}"


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
    args = sys.argv[1:]
    global ROUNDS
    bf16 = x3 = False
    if "--precision" in args:
        i = args.index("--precision")
        if args[i + 1:i + 2] not in (["bf16"], ["bf16x3"], ["fp32"]):
            sys.exit("--precision takes fp32, bf16 or bf16x3")
        bf16, x3 = args[i + 1] == "bf16", args[i + 1] == "bf16x3"
        del args[i:i + 2]
    batches = [int(a) for a in args] or [8, 4096]
    names = ["ours", "plain torch"]
    if bf16:
        names = ["ours-bf16", "ours-fp32", "torch-fp32", "torch-autocast-bf16"]
    if x3:
        names, ROUNDS = ["ours-bf16x3", "ours-fp32", "ours-bf16", "torch-fp32"], 7
    print(f"device {torch.cuda.get_device_name(0)}; L={L} E={E} heads={H} layers={LAYERS}; times in ms ({' / '.join(names)}), "
          "median of alternating rounds")

    def line(B, what, t, c, note=""):
        print(f"B={B}: {what:<29s} {' / '.join(f'{v:9.3f}' for v in t)}   sclk {c}{note}")

    for B in batches:
        torch.manual_seed(0)
        ours = GPTBackbone(E, L).cuda()
        ref = TorchBackbone(ours)
        mods = [ours, ref]                                              # the callables below, in the order of `names`
        extra = ()                                                      # further modules of ours, with their own mode
        if x3:
            ours3 = GPTBackbone(E, L).cuda().set_matmul_precision("bf16x3")
            ours16 = GPTBackbone(E, L).cuda().set_matmul_precision("bf16")
            ours3.load_state_dict(ours.state_dict())
            ours16.load_state_dict(ours.state_dict())
            mods, extra = [ours3, ours, ours16, ref], (ours3, ours16)
        if bf16:
            ours16 = GPTBackbone(E, L).cuda().set_matmul_precision("bf16")
            ours16.load_state_dict(ours.state_dict())
            extra = (ours16,)

            def ref16(x):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return ref(x).float()
            ref16.zero_grad = ref.zero_grad
            mods = [ours16, ours, ref, ref16]
        x = torch.randn(B, L, E, device="cuda")
        n = 300 if B <= 64 else 4
        for m in (ours, ref) + extra:
            m.eval()
        with torch.no_grad():
            base = ref(x)
            d = [((m(x) - base).abs().max() / base.abs().max()).item() for m in mods]
            t, c = alternate([lambda m=m: m(x) for m in mods], n)
            line(B, "eval forward, eager", t, c, "   (max rel diff to torch-fp32: " + " / ".join(f"{v:.1e}" for v in d) + ")")
            graphs = []
            for m in mods:
                if isinstance(m, GPTBackbone):
                    g = GraphedGPTBackbone(m, x)
                    graphs.append((lambda g=g: g(x), torch.equal(g(x), m(x))))
                else:
                    g = torch.cuda.CUDAGraph()
                    for _ in range(3):
                        m(x)
                    torch.cuda.synchronize()
                    with torch.cuda.graph(g):
                        m(x)
                    graphs.append((g.replay, None))
            t, c = alternate([g for g, _ in graphs], n)
            line(B, "eval forward, graph replay", t, c, f"   (replay == eager: {[s for _, s in graphs if s is not None]})")
        for m in (ours, ref) + extra:
            m.train()

        def step(m):
            m.zero_grad(set_to_none=True)
            m(x).square().mean().backward()
        t, c = alternate([lambda m=m: step(m) for m in mods], max(2, n // 2))
        line(B, "forward + backward, eager", t, c)
        replays = [graphed_step(m, x) for m in mods]
        t, c = alternate(replays, max(2, n // 2))
        line(B, "forward + backward, graph", t, c)
        del ours, ref, mods, x, replays, graphs, base, extra
        if bf16:
            del ours16, ref16
        if x3:
            del ours3, ours16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
