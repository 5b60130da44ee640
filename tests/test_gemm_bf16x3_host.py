"""CPU: the yardstick of the bf16x3 Linear tests and the host side of the mode, before any GPU run.

The references of tests/gemm_bf16x3_ref.py are held to what the GPU test assumes of them: the split is exact, an fp32
product of the split operands (the arithmetic the kernel does, in some order) stays within ONE any-order round-to-nearest
bound of the float64 three-term product, that product stays within 3 2^-16 (1 + 2^-7) R_exact of the exact one, and -- for
reductions of at most 136 -- a plain bf16 product violates the combined bound in more than three quarters of the elements, so
that bound tells the two modes apart there.  Then the switch, and the argument checks of the three new entry points (sizes are
checked before pointers, so null pointers do on a host without a GPU)."""
import pytest
import torch

import gemm_bf16_cases as C
import gemm_bf16x3_ref as X

CASES = X.all_cases()


def test_split_is_exact_and_meets_the_stated_bounds():
    torch.manual_seed(3)
    t = torch.cat([torch.randn(4096), torch.randn(4096) * 1e30, torch.randn(4096) * 1e-30,
                   torch.tensor([0.0, -0.0, 1.0, X.WITNESS_VALUE, C.TIE_EVEN_DOWN, C.TIE_EVEN_UP, C.TWO126, -C.TWO126])])
    hi, lo = X.split(t)                                                        # asserts the exactness of t - hi
    v = t.double()
    assert bool(((v - hi).abs() <= 2.0 ** -8 * v.abs()).all())
    assert bool(((v - hi - lo).abs() <= 2.0 ** -16 * v.abs()).all())
    assert bool((lo.abs() <= 2.0 ** -8 * (1 + 2.0 ** -8) * v.abs()).all())
    assert torch.equal(hi.float().bfloat16().double(), hi) and torch.equal(lo.float().bfloat16().double(), lo)
    w = X.split(torch.tensor([X.WITNESS_VALUE]))
    assert float(w[0]) == 1.0 and float(w[1]) == 2.0 ** -9
    bad = torch.tensor([float("nan"), float("inf"), float("-inf"), C.FLT_MAX, -C.FLT_MAX])
    hi, lo = X.split(bad)
    assert not bool(torch.isfinite(hi).any()) and bool((lo == 0).all())       # hi not finite: lo = 0


@pytest.mark.parametrize("case", CASES, ids=X.case_id)
def test_reference_products_meet_their_bounds(case):
    layout, N, K, J = case
    r = X.ref(layout, N, K, J)
    L = r["L"]
    # an fp32 product of the split operands: within 1 x the any-order RN bound of s3
    got = X.concat_fp32(layout, r["A"], r["B"]).double()
    rn = (3 * L + 1) * X.EPS * r["R3"]
    worst = float(((got - r["s3"]).abs() / rn.clamp_min(1e-300)).max())
    # s3 against the exact product
    e3 = float(((r["s3"] - r["exact"]).abs() / r["R_exact"].clamp_min(1e-300)).max())
    # a plain bf16 product against the combined bound
    viol = float(((r["plain"] - r["exact"]).abs() > X.combined_bound(L, r["R_exact"], r["R3"])).double().mean())
    print(f"{X.case_id(case)} L={L}: fp32 concat / RN bound = {worst:.3f}; |s3 - exact| / R_exact = {e3:.2e} "
          f"(bound {X.SPLIT_REL:.2e}); plain bf16 outside the combined bound in {viol:.2f} of the elements")
    assert worst <= 1.0
    assert e3 <= X.SPLIT_REL
    if L <= 136:
        assert viol > 0.75, "the combined bound does not tell bf16x3 from bf16 here"


def test_witness_values_are_what_the_split_gives():
    for fa, fb in ((True, True), (True, False), (False, True)):
        x, W, g = X.witness_operands("NT", 3, 40, 8, fa, fb)
        s3, _ = X.product3("NT", x, W)
        assert bool((s3 == X.witness_value(40, fa, fb)).all())
        assert bool((C.product64("NT", x, W)[0] == 40).all())                  # plain bf16 gives L
    assert X.witness_value(20001, True, True) == 20001 * (1 + 2.0 ** -8)
    assert torch.tensor(X.witness_value(20001, True, True), dtype=torch.float32).double() == X.witness_value(20001, True, True)


def test_backbone_switch_accepts_bf16x3():
    from lipvq_vae_amd.gpt import GPTBackbone
    net = GPTBackbone(64, 12, num_layers=1, num_heads=4)
    keys = list(net.state_dict().keys())
    assert net.set_matmul_precision("bf16x3") is net and net.matmul_precision == "bf16x3"
    assert list(net.state_dict().keys()) == keys
    with pytest.raises(ValueError, match="fp16"):
        net.set_matmul_precision("fp16")
    assert net.matmul_precision == "bf16x3"                                   # a refused value changes nothing
    assert net.set_matmul_precision("bf16").matmul_precision == "bf16"
    assert net.set_matmul_precision("fp32").matmul_precision == "fp32"


def test_linear_fn_names_a_refused_precision():
    from lipvq_vae_amd.nnfn import LinearFn
    x, W = torch.zeros(2, 8), torch.zeros(8, 8)
    for bad in ("fp16", "bf16x6", "BF16X3"):
        with pytest.raises(ValueError, match=bad):
            LinearFn.apply(x, W, None, 0, bad)


def test_new_entry_points_report_their_limits_without_a_gpu():
    from lipvq_vae_amd import _capi
    lib = _capi.lib

    def fwd(N, K, J):
        return lib.lipvq_linear_act_bf16x3(None, None, None, None, None, N, K, J, 0, None)

    def nn(N, J, K):
        return lib.lipvq_linear_nn_bf16x3(None, None, None, N, J, K, None)

    def wg(N, J, K):
        return lib.lipvq_wgrad_bf16x3(None, None, None, None, None, N, J, K, None)

    for call, name in ((fwd, b"lipvq_linear_act_bf16x3"), (nn, b"lipvq_linear_nn_bf16x3"), (wg, b"lipvq_wgrad_bf16x3")):
        assert call(240, 12, 64) == -2 and b"multiples of 8" in lib.lipvq_last_error() and name in lib.lipvq_last_error()
        assert call(240, 64, 12) == -2 and b"multiples of 8" in lib.lipvq_last_error()
        assert call(0, 64, 64) == 0                                           # zero rows: no-op
        assert call(-1, 64, 64) == -1 and call(4, 0, 64) == -1
        assert call(240, 64, 64) == -1 and b"null" in lib.lipvq_last_error()  # limits pass, then the pointers
    assert lib.lipvq_linear_act_bf16x3(None, None, None, None, None, 4, 64, 64, 7, None) == -1   # not an activation
