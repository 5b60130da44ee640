"""Host test of tests/backward_edge_cases.py, the case builders of tests/test_gpu_backward_extent.py: no GPU, no library.
The exact-sum bound, the int64 references, the poison maps against what stock fp32 torch on the CPU does, and that every case the
GPU file parametrizes over can be built (the GPU file imports its lists from the builder module: these are the same lists)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import backward_edge_cases as B  # noqa: E402
import backward_ref as R  # noqa: E402


def test_chunk_rows_and_exactness_bound():
    assert len(B.CHUNK_N) == 14 and list(B.CHUNK_N) == sorted(set(B.CHUNK_N))
    for n in B.CHUNK_N:
        assert 6 * n < 2 ** 24
    # the edges each entry names, from the restated chunking
    assert B.wgrad_chunks(128) == 1 and B.wgrad_chunks(129) == 3
    assert [B.wgrad_chunks(n) for n in (64 * 31 + 1, 64 * 32, 64 * 32 + 1, 64 * 96, 64 * 96 + 1, 64 * 97 + 1)] == [32, 32, 33, 96, 97, 98]
    assert [B.wgrad_chunk_rows(n) for n in (16383, 16384, 262143, 262144)] == [64, 256, 256, 1024]
    assert [B.wgrad_chunks(n) for n in (16383, 16384, 16385, 262143, 262144, 262145)] == [256, 64, 65, 1024, 256, 257]
    with pytest.raises(AssertionError):
        B.integer_wgrad_case(2 ** 24 // 6 + 1, 1, 1, 0)


@pytest.mark.parametrize("N,J,Kd,gather", [(129, 32, 32, False), (2049, 64, 100, False), (16385, 64, 100, True), (128, 32, 32, True)])
def test_integer_case_reference_equals_a_float64_product(N, J, Kd, gather):
    c = B.integer_wgrad_case(N, J, Kd, 7, gather)
    G, H = c["G"], c["H"]
    assert G.dtype == torch.float32 and H.dtype == torch.float32
    rows = H if c["hidx"] is None else H[c["hidx"]]
    assert bool((G == G.round()).all()) and float(G.abs().max()) == 2 and bool((rows == rows.round()).all()) and float(rows.abs().max()) == 3
    assert bool((G[:, 0] == 1).all()) and bool((rows[:, 0] == 1).all())
    if gather:
        used = torch.zeros(H.shape[0], dtype=torch.bool)
        used[c["hidx"]] = True
        assert 1 < int(used.sum()) < H.shape[0] and c["hidx"].unique().numel() < N and bool((H[~used] == 1e30).all())
    for act in (B.ACT_NONE, B.ACT_RELU):
        refW, refb = R.wgrad_ref(G, H, act, c["hidx"])
        assert c["gW"][act].dtype == torch.int64 and torch.equal(c["gW"][act].double(), refW)
        assert torch.equal(c["gW"][act].float().double(), refW)                   # ... and exactly representable in fp32
    assert torch.equal(c["gb"].double(), refb)
    assert int(c["gb"][0]) == N and int(c["gW"][B.ACT_NONE][0, 0]) == N and int(c["gW"][B.ACT_RELU][0, 0]) == N
    # any order gives the same fp32 bits: a shuffled fp32 product
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1))
    assert torch.equal(G[perm].t() @ rows[perm], c["gW"][B.ACT_NONE].float())


@pytest.mark.parametrize("N", B.POISON_N)
def test_wgrad_poison_maps_equal_what_fp32_torch_produces(N):
    J, Kd = 12, 9
    G, H = B.wgrad_case(N, J, Kd, N)
    G[:, 3] = 0.0                                                   # zeros in G: Inf * 0 = NaN must be in the map
    clean = (G.t() @ H, G.sum(0))
    for n in B.poison_rows(N):
        Gp = G.clone()
        Gp[n, 5] = float("nan")
        cW, cb = B.wgrad_poison_map(Gp, H, n)
        assert torch.equal(torch.isnan(cW), torch.arange(J)[:, None].expand(J, Kd) == 5) and torch.equal(torch.isnan(cb), torch.arange(J) == 5)
        got = (Gp.t() @ H, Gp.sum(0))
        assert torch.equal(torch.isnan(got[0]), torch.isnan(cW)) and torch.equal(torch.isnan(got[1]), torch.isnan(cb))
        assert torch.isfinite(got[0][cW == 0]).all() and torch.isfinite(got[1][cb == 0]).all()
        Hp = H.clone()
        Hp[n, 4] = float("inf")
        cW, cb = B.wgrad_poison_map(G, Hp, n)
        assert bool((cb == 0).all()) and bool((cW[:, [k for k in range(Kd) if k != 4]] == 0).all())
        assert bool(torch.isnan(cW[3, 4])) and bool(torch.isinf(cW[[j for j in range(J) if j != 3], 4]).all())
        got = G.t() @ Hp
        assert torch.equal(torch.isnan(got), torch.isnan(cW))
        inf = torch.isinf(cW)
        assert torch.equal(got[inf].double(), cW[inf])
        assert torch.isfinite(got[cW == 0]).all()
        assert torch.equal(G.sum(0), clean[1])


def _mlp3_bwd_fp32(gy, pre, W0, W1, W2, acts):
    """A plain three-layer backward chain in stock fp32 torch on the CPU."""
    d = [R.act_grad_ref(p, a).float() if p is not None else None for p, a in zip(pre, acts)]
    g2 = gy if d[2] is None else gy * d[2]
    g1 = (g2 @ W2) * d[1]
    g0 = (g1 @ W1) * d[0]
    return g2, g1, g0, g0 @ W0


@pytest.mark.parametrize("acts", [B.ENC, B.DEC, B.RELU3])
def test_mlp3_poison_map_equals_what_fp32_torch_produces(acts):
    case = B.mlp3_bwd_case(70, 7, 64, 128, 5, acts)
    clean = _mlp3_bwd_fp32(case["gy"], case["pre"], *case["W"], acts)
    for row in B.mlp3_isolation_rows(70):
        masks = B.mlp3_poison_map(case, row, 2)
        gy = case["gy"].clone()
        gy[row, 2] = float("nan")
        got = _mlp3_bwd_fp32(gy, case["pre"], *case["W"], acts)
        for g, c, m, name in zip(got, clean, masks, ("g2", "g1", "g0", "gx")):
            assert torch.equal(torch.isnan(g), m), name
            assert torch.equal(g[~m], c[~m]), name                  # row-wise products: the other rows keep their bits
        assert int(masks[0].sum()) == 1 and bool(masks[0][row, 2])
        for m in masks[1:]:
            assert bool(m[row].all()) and int(m.sum()) == m.shape[1]


def test_every_gpu_case_is_buildable():
    assert len(B.EXACT_SUM_CASES) == len(B.CHUNK_N) * 4 + sum(n <= B.GATHER_MAX_N for n in B.CHUNK_N) * 4
    for N, J, Kd, act, gather in B.EXACT_SUM_CASES:
        assert N in B.CHUNK_N and (J, Kd) in B.EXACT_JK and act in (B.ACT_NONE, B.ACT_RELU) and 6 * N < 2 ** 24
    c = B.integer_wgrad_case(B.CHUNK_N[-1], 64, 100, 3)            # the largest one builds, and counts its rows
    assert int(c["gb"][0]) == B.CHUNK_N[-1] and c["G"].shape == (B.CHUNK_N[-1], 64)
    assert {(j, k) for _, j, k, m in B.WGRAD_EXTENT_CASES if m == "plain"} == {(j, k) for j, k, _ in B.WGRAD_EXTENT_SHAPES}
    assert {m for *_, m in B.WGRAD_EXTENT_CASES} == {"plain", "nobias", "misaligned", "offset_out"}
    for N, J, Kd, _ in B.WGRAD_EXTENT_CASES:
        G, H = B.wgrad_case(N, J, Kd, 1)
        assert G.shape == (N, J) and H.shape == (N, Kd)
    for N in B.POISON_N:
        rows = B.poison_rows(N)
        assert rows[0] == 0 and rows[-1] == N - 1 and len(set(rows)) == len(rows)
        if N > 128:
            assert 63 in rows and 64 in rows
    for _, dims, mode in B.MLP3_EXTENT_CASES:
        N, K0, J0, J1, J2, acts = dims
        assert mode in ("plain", "no_g2", "no_gx", "offset_out") and (mode != "no_g2" or acts[2] == B.ACT_NONE)
    for _, dims in B.MLP3_ISOLATION_CASES[:2] + [("small", (33, 209, 64, 128, 5, B.ENC))]:
        case = B.mlp3_bwd_case(*dims)
        assert case["gy"].shape == (dims[0], dims[4]) and (case["pre"][2] is None) == (dims[5][2] == B.ACT_NONE)
        for row in B.mlp3_isolation_rows(dims[0]):
            assert [m.shape for m in B.mlp3_poison_map(case, row, 0)] == [(dims[0], w) for w in (dims[4], dims[3], dims[2], dims[1])]
    assert B.mlp3_isolation_rows(B.LDS_N) == [0, 31, 32, B.LDS_N - 1]
    for term, a_form, b_form in B.VQ_FORMS:
        assert term in B.VQ_DIMS and b_form in ("rows", "table") and (a_form is None) == (term == "in")
    c = B.vq_case("out", 5)
    assert c["x"].shape == (B.LDS_ROWS, 64) and c["a_idx"].shape == (B.LDS_ROWS,) and int(c["a_idx"].max()) < B.VQ_TABLE_ROWS
    assert all(n >= 1 for n in B.ACT_BWD_N + B.SDIFF_N) and 1 in B.ACT_BWD_N and 1 in B.SDIFF_N
    assert all(1 <= d and 1 <= h <= B.LIPB_HMAX for d, h in B.LIPB_DH)


@pytest.mark.parametrize("J,K", B.SPECTRAL_JK)
@pytest.mark.parametrize("training", [True, False])
def test_spectral_budget_holds_for_fp32_torch(J, K, training):
    """The derived budgets against stock fp32 torch on the CPU running the same formulas (its dot products are in another order
    than the kernel's chains; dot_bound holds for any order)."""
    import torch.nn.functional as F
    c = B.spectral_case(J, K, J + K)
    ref = B.spectral_ref_and_budget(c["W"], c["u"], c["v"], training)
    W, u, v = c["W"], c["u"], c["v"]
    if training:
        v = F.normalize(torch.mv(W.t(), u), dim=0, eps=B.SPECTRAL_EPS)
        u = F.normalize(torch.mv(W, v), dim=0, eps=B.SPECTRAL_EPS)
    sigma = torch.dot(u, torch.mv(W, v))
    for got, key in ((u, "u"), (v, "v"), (sigma, "sigma"), (W / sigma, "Wsn")):
        err = (got.double() - ref[key]).abs()
        assert bool((err <= ref["d_" + key]).all()), (key, float((err / ref["d_" + key]).max()))
    gref, allowed = B.spectral_bwd_ref_and_budget(c["gWsn"], W / sigma, u, v, sigma)
    dot = ((c["gWsn"].double() * (W / sigma).double()).sum()).float()
    got = (c["gWsn"] - dot * torch.outer(u, v)) / sigma
    assert bool(((got.double() - gref).abs() <= allowed).all())


def test_spectral_degenerate_cases():
    c = B.spectral_case(64, 7, 3, "rank_one")
    ref = B.spectral_ref_and_budget(c["W"], c["u"], c["v"], True)
    assert abs(float(ref["sigma"]) - c["sigma_exact"]) <= 2 * R.U32 * c["sigma_exact"]
    z = B.spectral_case(5, 4, 3, "zero")
    assert bool((z["W"] == 0).all())
    assert B.value_class(torch.tensor([1.5, 0.0, -0.0, float("nan"), float("inf"), float("-inf")])).tolist() == [0, 1, 1, 2, 3, 4]
