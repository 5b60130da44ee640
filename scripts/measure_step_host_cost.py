"""Dev tool (GPU): cost of one small eager call where the host, not the GPU, sets the pace -- LLFQVAE_V4(12, 208, 1024) at N = 80,
`tokenize` and one training step (`forward`, `backward`, no optimizer).  Five repeats of 2000 calls each, every repeat ending in a
synchronise; one JSON line.  To compare two Python trees on one library (a routing change), alternate processes:
    LIPVQ_HIP_LIBRARY=<build> python scripts/measure_step_host_cost.py [<root of the tree to import>] [<label>]"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
from lipvq_vae_amd.tokenizer import LLFQVAE_V4  # noqa: E402

torch.manual_seed(0)
m = LLFQVAE_V4(12, 208, 1024).cuda()
x = torch.randn(80, 12, device="cuda")
params = list(m.parameters())


def tok():
    m.tokenize(x)


def step():
    for p in params:
        p.grad = None
    m(x)[1].backward()


out = {"tree": sys.argv[2] if len(sys.argv) > 2 else "this"}
for name, fn in (("tokenize_us", tok), ("train_step_us", step)):
    for _ in range(500):
        fn()
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(2000):
            fn()
        torch.cuda.synchronize()
        reps.append(round((time.perf_counter() - t) / 2000 * 1e6, 3))
    out[name] = reps
print(json.dumps(out), flush=True)
