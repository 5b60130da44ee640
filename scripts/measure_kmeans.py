"""Dev tool (GPU): the k-means extension (csrc/lipvq_kmeans.hip, kmeans.py), HIP-event timed -- k-means++ seeding
(ops.kmeans_seed on the default seed subset of min(N, 256 K) rows) and one Lloyd step (kmeans.lloyd_step on all N rows) at cfg2
(K = 1024, D = 64), cfg3 (K = 8192, D = 128) and the ICRT shape (A = 12, D = 208, K = 1024), on the encoder outputs of an
LLFQVAE_V4 with trained-like parameters.  Per seeding pass: bytes of z read, the rate they were read at, against a device-to-device
copy measured in the same process (read + write bytes / time, warm).  One JSON line per shape.  Kernel-level numbers: run it
under `rocprofv3 --kernel-trace --stats -- python scripts/measure_kmeans.py` (a run of its own).

    python scripts/measure_kmeans.py [--shapes cfg2,cfg3,icrt] [--rows 524288] [--reps 3] [--out profiles/<name>.jsonl]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from oracle import lipvq_oracle as O

SHAPES = {"cfg2": (7, 64, 1024), "cfg3": (7, 128, 8192), "icrt": (12, 208, 1024)}     # (A, D, K)


def timed_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def copy_gbs():
    src = torch.empty(1 << 28, device="cuda", dtype=torch.float32)         # 1 GiB
    dst = torch.empty_like(src)
    ms = timed_ms(lambda: dst.copy_(src), 10, warmup=3)
    return 2 * src.numel() * 4 / ms / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg2,cfg3,icrt")
    ap.add_argument("--rows", type=int, default=524288)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lipvq_vae_amd import ops
    from lipvq_vae_amd.kmeans import draws, lloyd_step
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4
    orc = O.CanonicalOracle()
    hbm = copy_gbs()
    lines = []
    for name in args.shapes.split(","):
        A, D, K = SHAPES[name]
        p = O.make_params(7, A, D, K, oracle=orc)
        model = LLFQVAE_V4(A, D, num_codes=K).cuda()
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in p.items()})
        z = model.encode(torch.from_numpy(O.make_inputs(8, args.rows, A)).cuda())
        n_seed = min(args.rows, 256 * K)
        g = torch.Generator().manual_seed(0)
        zs = z.index_select(0, torch.randperm(args.rows, generator=g)[:n_seed].cuda())
        u = draws(K, g, z.device)
        cb = torch.empty(K, D, device="cuda")
        seed_ms = timed_ms(lambda: ops.kmeans_seed(zs, K, u, out=cb), args.reps)
        ops.kmeans_seed(zs, K, u, out=cb)
        work = cb.clone()
        lloyd_ms = timed_ms(lambda: (work.copy_(cb), lloyd_step(z, work, generator=g)), args.reps)
        pass_bytes = n_seed * D * 4
        per_centre_us = seed_ms * 1e3 / K
        rec = {"shape": name, "A": A, "D": D, "K": K, "rows": args.rows, "seed_rows": n_seed,
               "seed_ms": round(seed_ms, 3), "lloyd_step_ms": round(lloyd_ms, 3), "launches_per_centre": 2,
               "us_per_centre": round(per_centre_us, 2), "z_bytes_per_pass": pass_bytes,
               "z_read_GBs_per_centre": round(pass_bytes / (per_centre_us * 1e3), 1), "copy_GBs": round(hbm, 1)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del z, zs, model
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
