"""Dev tool (GPU): the tokenizer at latent widths 208 ... 512 (K = 1024, A = 12, trained-like parameters), HIP-event timed --
tokenize of 524 288 rows (and the share of rows the screen certified), an eager and a graphed training step at 80 and 500
rows.  One JSON line per width.  For a same-box A/B against another revision, build its library with scripts/ab_head.sh and
run this script again with LIPVQ_HIP_LIBRARY=build_ab/<name>/_lipvq_hip.so.

    python scripts/measure_wide.py [--widths 208,256,384,512] [--rows 524288] [--reps 5] [--out profiles/<name>.jsonl]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from oracle import lipvq_oracle as O


def timed_ms(fn, reps, warmup=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="208,256,384,512")
    ap.add_argument("--rows", type=int, default=524288)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lipvq_vae_amd import ops
    from lipvq_vae_amd.icl import GraphedTokenizerStep, VQTokenizerTrainer
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4
    A, K = 12, 1024
    orc = O.CanonicalOracle()
    lines = []
    for D in (int(w) for w in args.widths.split(",")):
        p = O.make_params(7, A, D, K, oracle=orc)
        model = LLFQVAE_V4(A, D, num_codes=K).cuda()
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in p.items()})
        x = torch.from_numpy(O.make_inputs(8, args.rows, A)).cuda()
        rec = {"D": D, "K": K, "A": A, "rows": args.rows,
               "screen_supported": ops.nearest_screen_supported(K, D), "fused": model.fused_shape()}
        rec["tokenize_ms"] = timed_ms(lambda: model.tokenize(x, count_usage=False), args.reps)
        model.tokenize(x, count_usage=False)
        torch.cuda.synchronize()
        ws = model.last_exact_rows
        rec["certified_share"] = None if ws is None else 1.0 - int(ws[0]) / args.rows
        del x
        for N in (80, 500):
            xs = torch.from_numpy(O.make_inputs(9 + N, N, A)).cuda()
            m = LLFQVAE_V4(A, D, num_codes=K).cuda()
            m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in p.items()})
            tr = VQTokenizerTrainer(m)
            rec[f"step{N}_eager_ms"] = timed_ms(lambda: tr.train_on_actions(xs), args.step_reps, warmup=3)
            g = GraphedTokenizerStep(m, xs, optimizer_state=tr.vq_optimizer.state_dict(), warmup=2)
            rec[f"step{N}_graphed_ms"] = timed_ms(lambda: g.step(xs), args.step_reps, warmup=3)
            del g, tr, m
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
