"""Dev measurement (GPU): ICLInputEmbedding and DefaultActionNetwork under their two dropout sources -- "torch" (nn.Dropout over
the finished [B, 3T, E] tensor; per encoder layer torch.rand + compare + cast for the attention bytes and three F.dropout) against
"kernel" (decisions drawn inside the HIP kernels, lipvq-vae_amd/csrc/lipvq_rng.h) -- same parameters, same GPU, same process.

    python scripts/bench_module_dropout.py
    python scripts/bench_module_dropout.py indexed      (the embedding's indexed backward alone: fixed-order route / the route before it)

Per module and shape: forward + backward, eager.  The two sides ALTERNATE window by window after a warm-up of both; the figure is
the median of 7 windows with their minimum and maximum beside it, and the shader clock (rocm-smi, read right after the timed
windows) is printed beside every line: a time without its clock does not compare across devices.
torch.cuda.max_memory_allocated of one forward + backward is reported for both sources.  Last, device events around the
attention kernels alone at S = 2048: lipvq_attention_drop_f32 against lipvq_attention_f32 with keep bytes PLUS the torch.rand /
compare / cast launches that make the bytes, and the two backward pairs."""
import json
import statistics
import subprocess
import sys
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

import lipvq_vae_amd  # noqa: E402,F401
from lipvq_vae_amd import ops  # noqa: E402
from lipvq_vae_amd.default_branch import DefaultActionNetwork  # noqa: E402
from lipvq_vae_amd.embedding import ICLInputEmbedding  # noqa: E402

E, T, DIN, D, A, H, P = 512, 10, 64, 208, 7, 8, 0.1
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
    lost = statistics.median(ta) > statistics.median(tb) and min(ta) > max(tb)          # slower by more than the windows' spread
    return statistics.median(ta), statistics.median(tb), f"{sclk()}   min-max {spread}", lost


def peak_mib(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def line(what, t_k, t_t, c, lost):
    note = "   **kernel source slower, beyond the spread**" if lost else ("   (kernel source slower, within the spread)" if t_k > t_t else "")
    print(f"{what}: kernel {t_k:9.3f} / torch {t_t:9.3f}   torch / kernel {t_t / t_k:5.2f}   sclk {c}{note}", flush=True)


def pair(what, make, step, n):
    nets = {s: make().set_dropout_source(s, seed=1 if s == "kernel" else None) for s in ("kernel", "torch")}
    t_k, t_t, c, lost = alternate(lambda: step(nets["kernel"]), lambda: step(nets["torch"]), n)
    line(f"{what}: forward + backward, eager", t_k, t_t, c, lost)
    m_k, m_t = peak_mib(lambda: step(nets["kernel"])), peak_mib(lambda: step(nets["torch"]))
    print(f"{what}: peak memory of one forward + backward above the resident tensors: kernel {m_k:9.1f} MiB / torch {m_t:9.1f} MiB "
          f"(torch - kernel = {m_t - m_k:.1f} MiB)", flush=True)
    del nets
    torch.cuda.empty_cache()


def embedding():
    torch.manual_seed(0)
    return ICLInputEmbedding(DIN, embed_dim=E, context_length=T, emb_dropout=P).cuda().train()


def default_branch():
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DefaultActionNetwork(A, D).cuda().train()


def main():
    print(f"device {torch.cuda.get_device_name(0)}; p={P}; times in ms, median of {WINDOWS} alternating windows", flush=True)
    for B in (8, 4096):
        obs, cobs, cact = (torch.randn(B, T, DIN, device="cuda") for _ in range(3))

        def step(net):
            net.zero_grad(set_to_none=True)
            net(obs, cobs, cact).square().mean().backward()
        pair(f"ICLInputEmbedding [{B}, {3 * T}, {E}]", embedding, step, 30 if B <= 64 else 3)
    for N in (80, 2048):
        x = torch.randn(N, A, device="cuda")

        def step(net):
            net.zero_grad(set_to_none=True)
            net(x).square().mean().backward()
        pair(f"DefaultActionNetwork N={N} D={D}", default_branch, step, 10 if N <= 256 else 3)
    # the attention kernels alone, S = 2048: drawn in the kernel against keep bytes + the launches that make the bytes
    S = 2048
    qkv, gout = torch.randn(S, 3 * D, device="cuda"), torch.randn(S, D, device="cuda")
    snap = ops.dropout_begin(torch.tensor([1, 0], dtype=torch.int64, device="cuda"))
    drop = (snap, ops.DROPOUT_SITE_DEFAULT, P)

    def fwd_bytes():
        keep = (torch.rand((H, S, S), device="cuda") >= P).to(torch.uint8)
        return ops.attention(qkv, H, keep, 1.0 - P)
    t_k, t_t, c, lost = alternate(lambda: ops.attention(qkv, H, dropout=drop), fwd_bytes, 5)
    line(f"attention forward S={S} D={D}: _drop kernel / keep-byte kernel + rand, compare, cast", t_k, t_t, c, lost)
    keep = (torch.rand((H, S, S), device="cuda") >= P).to(torch.uint8)
    t_k, t_t, c, lost = alternate(lambda: ops.attention(qkv, H, dropout=drop), lambda: ops.attention(qkv, H, keep, 1.0 - P), 5)
    line(f"attention forward S={S} D={D}: _drop kernel / keep-byte kernel alone (bytes given)", t_k, t_t, c, lost)
    out, lse = ops.attention(qkv, H, keep, 1.0 - P)
    t_k, t_t, c, lost = alternate(lambda: ops.attention_bwd(qkv, out, gout, lse, H, dropout=drop),
                                  lambda: ops.attention_bwd(qkv, out, gout, lse, H, keep, 1.0 - P), 5)
    line(f"attention backward S={S} D={D}: _drop kernels / keep-byte kernels (bytes given)", t_k, t_t, c, lost)


def indexed_backward():
    """embed_rows backward of an INDEXED stream: the fixed-order route ops.embed_rows_bwd takes (lipvq_embed_rows_bwd_det_f32)
    against the entry point the same call took before it (the workspace route where supported, else the atomic kernel)."""
    from lipvq_vae_amd._capi import check, lib
    from lipvq_vae_amd.ops import _ptr, _stream
    for B, K in ((8, 1024), (400, 1024), (2400, 1024), (2400, 32768), (4096, 1024), (4096, 32768)):
        N = B * T
        table, pos, w, b = (torch.randn(K, E, device="cuda"), torch.randn(T, E, device="cuda"), torch.ones(E, device="cuda"),
                            torch.zeros(E, device="cuda"))
        idx = torch.randint(0, K, (N,), device="cuda")
        out, gout = torch.zeros(B, 3 * T, E, device="cuda"), torch.randn(B, 3 * T, E, device="cuda")
        layout = (3 * T * E, 2 * E, E)
        stats = ops.embed_rows(table, idx, pos, w, b, 1e-5, out, N, T, *layout, want_stats=True)
        g = [torch.zeros_like(table), torch.zeros_like(pos), torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")]
        ws_ok = bool(lib.lipvq_embed_rows_bwd_ws_supported(N, T, E, K))
        ws = torch.empty(max(16, lib.lipvq_embed_rows_bwd_workspace_bytes(N, T, E, K)), device="cuda", dtype=torch.uint8)

        def before():
            head = (_ptr(gout), _ptr(table), _ptr(idx), _ptr(pos), _ptr(stats), _ptr(w), *(_ptr(t) for t in g))
            if ws_ok:
                check(lib.lipvq_embed_rows_bwd_ws_f32(*head, _ptr(ws), N, T, E, K, *layout, _stream()), "ws")
            else:
                check(lib.lipvq_embed_rows_bwd_f32(*head, N, T, E, K, *layout, _stream()), "atomic")
        t_k, t_t, c, lost = alternate(lambda: ops.embed_rows_bwd(gout, table, idx, pos, stats, w, *g, N, T, *layout), before, 10 if N <= 4096 else 3)
        note = "   **fixed-order route slower, beyond the spread**" if lost else ""
        print(f"embed_rows backward, indexed, N={N} K={K} E={E}: fixed-order {t_k:8.3f} / {'workspace' if ws_ok else 'atomic'} entry point "
              f"{t_t:8.3f}   sclk {c}{note}", flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["indexed"]:
        indexed_backward()
        sys.exit(0)
    main()
