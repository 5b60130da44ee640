"""CPU: the inputs of tests/test_gpu_scatter_edges.py can see what they are meant to see.  On each of them the numpy
restatement of the 256-row segment order (tests/scatter_ref.py) changes the bits of EVERY code concerned when the rows of a code
are taken in reverse, when the segment is 128 rows long, and when the segment sums are added in reverse -- so a kernel with any
of these faults cannot match it -- and it stays inside the float64 bound of test_scatter_add_sorted_route."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scatter_ref as S  # noqa: E402

CASES = {"order": S.order_case, "combine": S.combine_case}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    g, idx, K, gC0, counts = CASES[request.param]()
    return dict(g=g, idx=idx, K=K, gC0=gC0, counts=counts, ref=S.sorted_ref(g, idx, K), ref0=S.sorted_ref(g, idx, K, gC0))


def test_counts_are_as_stated():
    g, idx, K, gC0, counts = S.order_case()
    assert g.shape == (32768 + 13, 65) and K == 40 and gC0.shape == (K, 65)
    assert np.array_equal(np.bincount(idx, minlength=K), counts)
    assert tuple(counts[:19]) == S.ORDER_COUNTS and counts[19] > 20000
    pos = np.nonzero(idx == 18)[0]                               # shuffled: a code's rows span the blocks and waves
    assert pos.min() < 2048 and pos.max() > 30000
    g, idx, K, gC0, counts = S.combine_case()
    assert np.array_equal(np.bincount(idx, minlength=K), counts)
    assert tuple(-(-counts[1:6] // S.SEG)) == S.COMBINE_SEGMENTS and counts[5] == 16 * 256 + 1


def test_reversed_rows_change_every_code_of_three_rows_or_more(case):
    rev = S.sorted_ref(case["g"], case["idx"], case["K"], mutate="reverse_rows")
    differ = S.code_bits_differ(case["ref"], rev)
    assert (case["counts"] >= 3).sum() >= 8
    assert differ[case["counts"] >= 3].all()
    assert not differ[case["counts"] <= 2].any()                 # a + b = b + a; one row; none


def test_segment_of_128_rows_changes_every_code_above_256_rows(case):
    half = S.sorted_ref(case["g"], case["idx"], case["K"], seg=128)
    differ = S.code_bits_differ(case["ref"], half)
    assert (case["counts"] > 256).sum() >= 5
    assert differ[case["counts"] > 256].all()
    assert not differ[case["counts"] <= 128].any()


def test_reversed_segment_sums_change_every_code_of_two_segments_or_more(case):
    """With a non-zero gC0: (gC0 + s_0) + s_1 is not (gC0 + s_1) + s_0.  With gC0 = 0 two segments commute, three do not."""
    segs = -(-case["counts"] // S.SEG)
    rev0 = S.sorted_ref(case["g"], case["idx"], case["K"], case["gC0"], mutate="reverse_segments")
    differ0 = S.code_bits_differ(case["ref0"], rev0)
    assert (segs >= 2).sum() >= 5 and (segs == 2).any()
    assert differ0[segs >= 2].all() and not differ0[segs <= 1].any()
    rev = S.sorted_ref(case["g"], case["idx"], case["K"], mutate="reverse_segments")
    assert S.code_bits_differ(case["ref"], rev)[segs >= 3].all()


def test_gc0_is_seen_by_every_code(case):
    """A kernel that overwrote instead of accumulating, or dropped gC0 of an empty code, cannot match."""
    assert S.code_bits_differ(case["ref"], case["ref0"]).all()
    empty = case["counts"] == 0
    assert empty.any() and S.bits_equal(case["ref0"][empty], case["gC0"][empty])


def test_sequential_order_differs_from_the_segment_order(case):
    """Beyond one segment the two orders are different numbers: the routes cannot be mistaken for one another.  (From a
    non-zero gC0: with gC0 = 0 a code of 257 rows is s_0 + its last row in both orders.)"""
    seq = S.seq_ref(case["g"], case["idx"], case["K"], case["gC0"])
    differ = S.code_bits_differ(case["ref0"], seq)
    assert differ[case["counts"] > 256].all() and not differ[case["counts"] <= 1].any()


def test_restatement_is_inside_the_float64_bound(case):
    g, idx, K = case["g"], case["idx"], case["K"]
    ref64 = np.zeros((K, g.shape[1]), np.float64)
    np.add.at(ref64, idx, g.astype(np.float64))
    scale = float(np.abs(g).max()) * float(np.sqrt(max(1, case["counts"].max())))
    bound = 2e-6 * max(scale, float(np.abs(ref64).max()))       # test_scatter_add_sorted_route's
    assert np.abs(case["ref"].astype(np.float64) - ref64).max() <= bound
    assert np.abs(S.seq_ref(g, idx, K).astype(np.float64) - ref64).max() <= bound


def test_one_code_case_sees_segment_length_and_order():
    for code in (0, 1):
        g, idx, K, gC0 = S.one_code_case(code)
        ref = S.sorted_ref(g, idx, K, gC0)
        assert S.bits_equal(ref[1 - code], gC0[1 - code])
        for other in (S.sorted_ref(g, idx, K, gC0, seg=128), S.sorted_ref(g, idx, K, gC0, mutate="reverse_segments"),
                      S.sorted_ref(g, idx, K, gC0, mutate="reverse_rows"), S.seq_ref(g, idx, K, gC0)):
            assert S.code_bits_differ(ref, other)[code]


def test_fold_rows_rounds_three_times():
    """f * (t - z) + g in fp32 steps: differs from the fused and the float64 evaluations somewhere, equals the stepwise one."""
    rng = np.random.default_rng(0)
    N, K, D = 500, 7, 9
    g, ze, table = (rng.standard_normal(s).astype(np.float32) for s in ((N, D), (N, D), (K, D)))
    idx = rng.integers(0, K, N)
    alpha, gs = 0.37, np.float32(1.7)
    rows = S.fold_rows(g, ze, table, idx, alpha, gs)
    f = np.float32(np.float32(alpha) * gs)
    step = ((table[idx] - ze).astype(np.float32) * f).astype(np.float32) + g
    assert S.bits_equal(rows, step)
    wide = (np.float64(f) * (table[idx].astype(np.float64) - ze) + g).astype(np.float32)
    assert not S.bits_equal(rows, wide)
    assert S.bits_equal(S.fold_rows(None, ze, table, idx, alpha, None), np.float32(alpha) * (table[idx] - ze))
