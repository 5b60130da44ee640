"""CPU: the large-extent cases (tests/extent_cases.py) are what tests/test_gpu_large_extent.py takes them for -- the windows lie
inside the operand and straddle their boundaries, the operand crosses 2^31 elements, the declared device memory stays under the cap,
every call is legal under the library's own limits, the exact-sum operands are exact in fp32 in any summation order -- and the
workspace size functions of include/lipvq.h do not wrap up to N = 2^33."""
import numpy as np
import pytest

import dropout_ref
import extent_cases as X

CASE_IDS = [c.name for c in X.CASES]


def _lib():
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd._capi import lib
    return lib


def test_the_table_names_every_case_once():
    assert len(set(CASE_IDS)) == len(CASE_IDS) and len(X.CASES) >= 20


@pytest.mark.parametrize("case", X.CASES, ids=CASE_IDS)
def test_windows_boundaries_and_memory(case):
    N, W = case.N, case.W
    assert case.elems > X.B31 and N * W > max(case.boundaries)
    if case.name == "attention_unbatched":
        # S = 23 200 is the issue's: H S S = 4.31e9 bytes pass 2^32 by 10.8 M, that is 465 rows of S bytes and not the 549 of the rule
        assert N * W - X.B32 > 256 * W and N == X.XF_H * X.XF_S and W == X.XF_S
    elif W > 1:
        assert X.rows_for(W, max(case.boundaries)) <= N < X.rows_for(W, max(case.boundaries)) + 128      # (whole batches / sequences)
        # one complete tile of the largest kind wholly past the last boundary, and a ragged last tile
        first_tile_past = -(-(max(case.boundaries) // W + 1) // X.TILE_ROWS) * X.TILE_ROWS
        assert first_tile_past + X.TILE_ROWS <= N
        if "attention" not in case.name:                                # (a sequence is 128 rows: no ragged tile there)
            assert N % X.TILE_ROWS != 0 and N % 32 != 0
    else:
        assert N == max(case.boundaries) + X.FLAT_TAIL
    wins = X.windows(N, W, case.boundaries)
    assert len(wins) == 2 + len(case.boundaries) and wins[0] == (0, 64) and wins[-1] == (N - 101, N)
    for a, b in wins:
        assert 0 <= a < b <= N
    for (a, b), bound in zip(wins[1:-1], case.boundaries):
        assert b - a == 128
        assert a * W < bound - 63 * W and (b - 1) * W + (W - 1) >= bound + 63 * W          # 64 rows on each side of the boundary element
        assert a * W <= bound < b * W
    rows = X.window_rows(N, W, case.boundaries)
    assert rows[0] == 0 and rows[-1] == N - 1 and len(rows) <= 64 + 128 * len(case.boundaries) + 101
    # chunked calls: an extent the small-shape suite covers
    assert X.chunk_rows(W) * W <= X.CHUNK_ELEMS and X.chunk_rows(W) % X.TILE_ROWS == 0
    assert 0 < case.need <= X.MEM_CAP, (case.name, case.need / 2 ** 30)
    assert all(b > 0 for _, b in case.allocs)


@pytest.mark.parametrize("case", X.CASES, ids=CASE_IDS)
def test_the_call_is_legal(case):
    lib = _lib()
    limits = X.documented_limits(case)
    assert limits
    for what, holds in limits:
        assert holds, (case.name, what)
    rcs = X.probe(case, lib)
    for rc in ([] if rcs is None else rcs if isinstance(rcs, list) else [rcs]):
        assert rc == X.EINVAL, (case.name, rc, lib.lipvq_last_error())         # past the size checks, refused for its null pointers only
        assert b"null" in lib.lipvq_last_error()
    if case.entry == "lipvq_mlp3_f32" and case.name == "mlp3":
        assert lib.lipvq_mlp3_loss_supported(case.N, *case.dims) == 1               # the folded-loss launch takes this stack
        assert lib.lipvq_mlp3_loss_supported(case.N, *X.MLP_DIMS_WG) == 0           # ... and not the (32, 32) one: another kernel
    if case.entry == "lipvq_tokenize_f32":
        A, J0, J1, K = case.dims
        assert lib.lipvq_tokenize_supported(A, J0, J1, case.W, K) == 1 and lib.lipvq_nearest_screened_supported(K, case.W) == 1
        assert lib.lipvq_tokenize_workspace_bytes(case.N, case.W) <= dict(case.allocs)["workspace"]
    if case.entry == "lipvq_nearest_screened_f32":
        assert lib.lipvq_nearest_screened_supported(*case.dims) == 1
        assert lib.lipvq_nearest_workspace_bytes(case.N) <= 1 << 30
    if case.entry == "lipvq_scatter_add_f32":
        K, D = case.dims
        assert lib.lipvq_scatter_add_sorted_supported(case.N, K, D) == 1
        assert lib.lipvq_scatter_add_sorted_workspace_bytes(case.N, K, D) <= dict(case.allocs)["workspace"]
    if case.entry == "lipvq_wgrad_f32":
        J, Kd = case.dims
        assert lib.lipvq_wgrad_workspace_bytes(case.N, J, Kd) <= dict(case.allocs)["workspace"]
        # the same shapes run lipvq_wgrad_bf16 / _bf16x3: widths multiples of 8, at most 65535 row chunks, the workspace fits
        assert J % 8 == 0 and Kd % 8 == 0
        nbytes = lib.lipvq_wgrad_bf16_workspace_bytes(case.N, J, Kd)
        assert 0 < nbytes <= dict(case.allocs)["workspace"] and nbytes // ((J * Kd + J) * 4) <= 65535
        for fn in (lib.lipvq_wgrad_bf16, lib.lipvq_wgrad_bf16x3):
            assert fn(None, None, None, None, None, case.N, J, Kd, None) == X.EINVAL and b"null" in lib.lipvq_last_error()


def test_the_size_checks_do_refuse():
    """The probes above can tell a refusal from a pass: one row more than the in-kernel source can count is EUNSUPPORTED."""
    lib = _lib()
    assert lib.lipvq_act_bwd_drop_f32(None, None, None, None, 7, 0.3, X.B32, 2048, 1, None) == X.EUNSUPPORTED
    assert lib.lipvq_gpt_layernorm_f32(None, None, None, None, 1e-5, None, None, None, None, 8, 1028, None) == X.EUNSUPPORTED
    assert lib.lipvq_gpt_layernorm_bwd_drop_f32(None, None, None, None, None, None, 7, 0.2, None, None, None, None, None, X.B32, 1024,
                                                None) == X.EUNSUPPORTED
    assert lib.lipvq_dropout_keep_u8(None, 7, X.B32, 2048, 0.25, None, None) == X.EUNSUPPORTED


def test_exact_values_are_small_integers_and_not_degenerate():
    rows = X.window_rows(X.rows_for(2048), 2048)
    for salt in range(1, 8):
        v = X.exact_values(rows, 2048, salt)
        assert v.dtype == np.int64 and v.min() == -8 and v.max() == 8
        assert len(np.unique(v)) == 17 and abs(v.mean()) < 0.5
        assert np.array_equal(v.astype(np.float32).astype(np.int64), v)
        # bf16 keeps 8 significant bits: |v| <= 8 survives the rounding
        assert np.array_equal((v.astype(np.float32).view(np.uint32) & 0xFFFF), np.zeros_like(v, np.uint32))
    assert not np.array_equal(X.exact_values(rows, 8, 1), X.exact_values(rows, 8, 2))
    assert not np.array_equal(X.exact_values(rows[:64], 8, 1), X.exact_values(rows[64:128], 8, 1))


def test_every_partial_sum_is_exact_in_fp32():
    bounds = X.exact_sum_bounds()
    assert len(bounds) >= 12
    for what, b in bounds.items():
        assert 0 < b < X.EXACT, (what, b)
    n = X.BY_NAME["mse_pair"].N
    s = X.mse_exact_sum(n)
    assert 0 < s < 2 ** 53 and isinstance(s, int)
    s = X.grad_exact_sumsq(X.BY_NAME["grad_norm"].N, 1000)
    assert 0 < s < 2 ** 53 and isinstance(s, int)


@pytest.mark.parametrize("indexed", [True, False])
def test_embed_rows_bwd_operands_are_exact(indexed):
    """Every value the backward forms on these operands is numerator / 1024 with |numerator| < 2^24, in any summation order."""
    case = X.BY_NAME["embed_rows_bwd"]
    x = X.embed_bwd_expected(case, indexed)
    T, B = case.dims
    assert len(x["n"]) >= 100 and x["n"].max() < B * T and x["n"].max() * case.W > X.B31 // 3       # rows of the last batches contribute
    assert len(np.unique(x["t"])) == T and 0 < x["bound"] < X.EXACT
    assert np.abs(x["g_pos"]).max() > 0 and np.abs(x["g_lnw"]).max() > 0
    lib = _lib()
    assert lib.lipvq_embed_rows_bwd_det_workspace_bytes(B * T, T, case.W, X.EMBED_K if indexed else B * T, int(indexed)) \
        <= dict(case.allocs)["workspace (row gradients, partial sums, sort)"]


def test_count_rows_and_codes():
    N = X.rows_for(208)
    rows = X.count_rows(N)
    assert rows[0] == 0 and len(rows) == -(-N // 8) and np.all(rows % 8 == 0)
    k = X.scatter_code(np.arange(N - 4096, N), 64)
    assert k.min() == 0 and k.max() == 63 and len(np.unique(k)) == 64        # rows past 2^31 elements land on every code


def test_keep_field_window_is_the_field():
    """dropout_ref.keep_field(row0=) is rows row0 ... of the field from row 0."""
    whole = dropout_ref.keep_field(5, 9, 3, 300, 40, 0.3)
    assert np.array_equal(dropout_ref.keep_field(5, 9, 3, 100, 40, 0.3, row0=200), whole[200:])
    assert np.array_equal(dropout_ref.keep_field(5, 9, 3, 300, 40, 0.3, row0=0), whole)
    far = dropout_ref.keep_field(5, 9, 3, 2, 8, 0.3, row0=2 ** 32 - 2)
    assert far.shape == (2, 8) and not np.array_equal(far, whole[:2, :8])


WS = X.workspace_exports()


@pytest.mark.parametrize("row", WS, ids=[f"{r[0]}-{'x'.join(map(str, r[1]))}" for r in WS])
def test_workspace_sizes_do_not_wrap(row):
    name, widths, call, floor, zero_is_refusal = row
    lib = _lib()
    last = 0
    seen = 0
    for N in X.WORKSPACE_NS:
        got = int(call(lib, N))
        if got == 0 and zero_is_refusal:
            continue                                        # documented: 0 = this N is refused
        seen += 1
        assert got >= last, (name, widths, N, got, last)    # a wrap shows up as a decrease
        assert got > 0, (name, widths, N)
        if floor is not None:
            assert got >= floor(N), (name, widths, N, got, floor(N))
        last = got
    assert seen >= 2, (name, widths)
