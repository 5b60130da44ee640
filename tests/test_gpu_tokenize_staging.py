"""GPU: the fused launch at latent widths <= 64 -- how the codebook stages travel to LDS and how the next row block's inputs are
prefetched (csrc/lipvq_screen.h lq_screen_core, csrc/lipvq_fused.hip load_x).  Where and when the bytes travel is a schedule; the
answers are the oracle's and the unfused route's (mlp3 + exact all-pairs nearest), bit for bit, at the smallest shapes at which each
piece of the schedule can go wrong:

  * stage counts: K = 37 pads to 256 codes = 2 stages at D = 32 (fewer than the ring runs ahead) and 4 at D = 64; 256 .. 2048 codes
    are 2 .. 32 stages; K = 2304 is past what the in-place decisions take (the launch stores z_e and lists its uncertified rows);
    K = 8192 under the three-product screen (an option; the one-product screen is that size's default) is 128 stages;
  * row counts 1, 31, 33, 256 and 2 * 256 + 37 (a ragged last block: one full wave, one with five rows, the rest empty);
  * a SECOND row block per workgroup -- more than 256 workgroups' worth of rows: the only launches in which the inputs prefetched
    behind the screen's first stage copies feed a following block;
  * fan-in 1, 2, 7, 12, 16 (prefetched: eight loads per lane, the ones past the fan-in masked where layer 0 consumes them) and 17
    (loaded at block start); one row of one float is the four-byte input, every clamped address of which is that one float;
  * the storing instances (the caller wants z_e) with the last tile's z_e stores in front of the screen and deferred behind its
    first copies, where stores (waves with a valid row only) and prefetch loads (every wave) are counted together.

A stage copy that lands late does not show in the answers: a row screened against stale bytes usually fails its certificate and is
then decided correctly in place.  It shows in `last_exact_rows`.  The screen's values are bit-identical from build to build, so the
count is a constant of the inputs: EXACT_ROWS holds the counts of the build this schedule was changed from (commit 40880ef), for
plain trained-like parameters (a fraction of a percent of the rows uncertified), measured on an MI355X with

    LIPVQ_HIP_LIBRARY=<that build's _lipvq_hip.so> python tests/test_gpu_tokenize_staging.py

which prints the dictionary below (seeds: torch.manual_seed(1000 + D), bench.trained_like_(seed=D), O.make_inputs(900 + K, N, 7)).
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import lipvq_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ["w8rg1", "w4rg1"]
N_RAGGED = 2 * 256 + 37
N_SECOND = {"w8rg1": 65536 + 256 + 37, "w4rg1": 32768 + 128 + 37}     # 256 workgroups x one row block, one more block, a ragged one
N_CONST = 65536 + 256 + 37

# (K, tok_shape) -> rows of the N_CONST-row launch left to an exact decision, D = 64, A = 7 (module docstring)
EXACT_ROWS = {
    (256, "w8rg1"): 177,
    (256, "w4rg1"): 177,
    (1024, "w8rg1"): 262,
    (1024, "w4rg1"): 262,
}

_cases = {}
_oracle = []


def _orc():
    if not _oracle:
        _oracle.append(O.CanonicalOracle())
    return _oracle[0]


def _case(A, D, K, dup=False):
    """(model on the GPU, its parameters as numpy arrays): bench.trained_like_ parameters as tests/test_gpu_tokenize_keepz.py builds
    them; dup: the upper half of the codebook overwritten by one-ulp copies of the lower half (every row a near-tie no screen can
    certify).  Built once per shape, never modified."""
    key = (A, D, K, dup)
    if key not in _cases:
        import bench
        from lipvq_vae_amd.tokenizer import LLFQVAE_V4
        torch.manual_seed(1000 + D)
        model = LLFQVAE_V4(A, D, num_codes=K).cuda()
        bench.trained_like_(model, A, seed=D)
        if dup:
            cb = model.quantizer.codebook.detach().cpu().numpy().copy()
            half = K // 2
            cb[half:2 * half] = cb[:half]
            j = np.arange(half) % D
            cb[half + np.arange(half), j] = np.nextafter(cb[np.arange(half), j], np.float32(2.0))
            with torch.no_grad():
                model.quantizer.codebook.copy_(torch.from_numpy(cb).cuda())
        p = {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in model.state_dict().items()}
        _cases[key] = (model, p)
    return _cases[key]


_refs = {}


def _reference(key, p, x):
    """the C oracle's (z_e, idx, usage) of one (parameters, inputs) pair: computed once, shared, never modified"""
    if key not in _refs:
        ze = _orc().llfq_encode(p, x)
        idx, _, usage = _orc().nearest(ze, p["quantizer.codebook"])
        _refs[key] = (ze, idx, usage)
    return _refs[key]


def _launch(model, xt):
    """model.tokenize (the caller wants no z_e) -> idx, zq, usage, rows decided by an exact stage"""
    model.reset_usage()
    idx, zq = model.tokenize(xt)
    return idx, zq, model.code_usage.clone(), int(model.last_exact_rows[0])


def _check(model, p, x, ref_key, storing=True):
    """The fused launch (twice: same answers, same number of uncertified rows) and the storing instance against the oracle and
    against the unfused route, everything with ==.  -> rows left to an exact decision"""
    from lipvq_vae_amd import ops
    N = x.shape[0]
    xt = torch.from_numpy(x).cuda()
    cb = model.quantizer.codebook.detach()
    ze_ref, idx_ref, usage_ref = _reference(ref_key, p, x)
    idx, zq, usage, exact = _launch(model, xt)
    idx2, zq2, usage2, exact2 = _launch(model, xt)
    print(f"N={N} A={x.shape[1]} D={model.latent_dim} K={model.num_codes}: exact rows {exact}, {exact2}")
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert torch.equal(zq, cb[idx])
    assert int(usage.sum()) == N and np.array_equal(usage.cpu().numpy(), usage_ref)
    assert torch.equal(idx2, idx) and torch.equal(zq2, zq) and torch.equal(usage2, usage) and exact2 == exact
    # the unfused route
    ze_u = model.encode(xt)
    idx_u, zq_u, _ = ops.nearest(ze_u, cb, ops.DIST_NORM)
    assert np.array_equal(ze_u.cpu().numpy(), ze_ref)
    assert torch.equal(idx_u, idx) and torch.equal(zq_u, zq)
    if storing:
        idx_s, zq_s, ze_s = model._tokenize_fused(xt, None, want_ze=True)
        assert torch.equal(idx_s, idx) and torch.equal(zq_s, zq)
        assert torch.equal(ze_s, ze_u)
    return exact


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("K", [37, 256, 512, 1024, 2048])
def test_stage_counts(lipvq_option, no_screen_monitor, K, D, shape):
    """2 .. 32 stages of the ring (K = 37 at D = 32: fewer stages than the ring runs ahead), plain trained-like parameters: the
    screen certifies most rows, so a wrong stage shows in the answers or in the count of the second launch."""
    model, p = _case(7, D, K)
    lipvq_option("tok_shape", shape)
    x = O.make_inputs(100 + K + D, N_RAGGED, 7)
    _check(model, p, x, ("stages", K, D))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D", [32, 64])
def test_codebook_past_the_inplace_limit(lipvq_option, no_screen_monitor, D, shape):
    """K = 2304 > 2048: no in-place decisions -- the launch that stores z_e and lists its uncertified rows."""
    K = 2304
    model, p = _case(7, D, K)
    lipvq_option("tok_shape", shape)
    x = O.make_inputs(200 + D, N_RAGGED, 7)
    _check(model, p, x, ("past", K, D))


@pytest.mark.parametrize("shape", SHAPES)
def test_large_codebook_under_the_three_product_screen(lipvq_option, no_screen_monitor, shape):
    """K = 8192 with screen_mode = fine: 128 stages at D = 64 through the same ring, 256 tiles' worth of code norms (more than
    the LDS could hold resident beside the encoder's weights and the ring)."""
    D, K = 64, 8192
    model, p = _case(7, D, K)
    lipvq_option("tok_shape", shape)
    lipvq_option("screen_mode", "fine")
    x = O.make_inputs(250, N_RAGGED, 7)
    _check(model, p, x, ("nofit", K, D))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("N", [1, 31, 33, 256, N_RAGGED])
def test_ragged_row_counts(lipvq_option, no_screen_monitor, N, shape):
    """every row a near-tie (duplicated codes): the in-place path on all of them, at every row count"""
    D, K = 64, 1024
    model, p = _case(7, D, K, dup=True)
    lipvq_option("tok_shape", shape)
    x = O.make_inputs(300 + N, N, 7)
    exact = _check(model, p, x, ("ragged", N))
    assert exact > N // 4


@pytest.mark.parametrize("defer", [None, "0", "1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_second_block_per_workgroup(lipvq_option, no_screen_monitor, shape, defer):
    """256 workgroups, then one more full row block and a ragged one: workgroups 0 and 1 run a second block on inputs prefetched
    behind the first block's stage copies.  defer = None: the launch without z_e; "0" / "1": the storing instance with its last
    tile's stores in front of the screen / behind its first copies (counted together with the loads)."""
    D, K = 64, 256
    model, p = _case(7, D, K)
    lipvq_option("tok_shape", shape)
    N = N_SECOND[shape]
    x = O.make_inputs(400, N_SECOND["w8rg1"], 7)[:N]
    ze_ref, idx_ref, usage_ref = _reference(("second", N), p, x)
    xt = torch.from_numpy(x).cuda()
    if defer is None:
        idx, zq, usage, exact = _launch(model, xt)
        print(f"N={N} {shape}: exact rows {exact}")
        assert np.array_equal(usage.cpu().numpy(), usage_ref)
    else:
        lipvq_option("tok_defer_ze", defer)
        idx, zq, ze = model._tokenize_fused(xt, None, want_ze=True)
        assert np.array_equal(ze.cpu().numpy(), ze_ref)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert torch.equal(zq, model.quantizer.codebook.detach()[idx])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("A,N", [(1, 1), (1, N_RAGGED), (2, N_RAGGED), (7, 1), (12, N_RAGGED), (16, N_RAGGED), (17, N_RAGGED)])
def test_row_widths(lipvq_option, no_screen_monitor, A, N, shape):
    """fan-in up to 16 is prefetched, 17 is not; (1, 1) is the four-byte input"""
    D, K = 64, 256
    model, p = _case(A, D, K)
    lipvq_option("tok_shape", shape)
    x = O.make_inputs(500 + A, N, A)
    _check(model, p, x, ("widths", A, N))


@pytest.mark.parametrize("defer", ["0", "1"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("rem", [1, 32, 33, 224])
def test_storing_instance_with_empty_waves(lipvq_option, no_screen_monitor, rem, shape, defer):
    """The storing instance, last row block with one valid wave up to all but one: a wave without a valid row issues no deferred
    store and counts none, but it does issue and count its prefetch loads."""
    D, K = 64, 1024
    model, p = _case(7, D, K, dup=True)
    lipvq_option("tok_shape", shape)
    lipvq_option("tok_defer_ze", defer)
    N = 256 + rem
    x = O.make_inputs(600 + rem, N, 7)
    ze_ref, idx_ref, _ = _reference(("storing", rem), p, x)
    idx, zq, ze = model._tokenize_fused(torch.from_numpy(x).cuda(), None, want_ze=True)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    assert np.array_equal(ze.cpu().numpy(), ze_ref)
    assert torch.equal(zq, model.quantizer.codebook.detach()[idx])


def _exact_rows_const(K, shape, set_option):
    """the two counts of the module docstring's launch, and its indices"""
    model, _ = _case(7, 64, K)
    set_option("tok_shape", shape)
    xt = torch.from_numpy(O.make_inputs(900 + K, N_CONST, 7)).cuda()
    idx, _, _, e1 = _launch(model, xt)
    idx2, _, _, e2 = _launch(model, xt)
    assert torch.equal(idx, idx2)
    return e1, e2, idx


@pytest.mark.parametrize("K,shape", sorted(EXACT_ROWS))
def test_no_late_copy_behind_the_exact_stage(lipvq_option, no_screen_monitor, K, shape):
    """Rows screened against bytes still in flight would be decided in place and answer correctly: the count gives them away."""
    from lipvq_vae_amd import ops
    e1, e2, idx = _exact_rows_const(K, shape, lipvq_option)
    print(f"K={K} {shape}: exact rows {e1}, {e2}; recorded {EXACT_ROWS[(K, shape)]}")
    assert e1 == e2
    assert e1 == EXACT_ROWS[(K, shape)]
    model, _ = _case(7, 64, K)
    xt = torch.from_numpy(O.make_inputs(900 + K, N_CONST, 7)).cuda()
    idx_u, _, _ = ops.nearest(model.encode(xt), model.quantizer.codebook.detach(), ops.DIST_NORM, want_zq=False)
    assert torch.equal(idx_u, idx)


if __name__ == "__main__":
    # prints EXACT_ROWS for the library in use (module docstring)
    import lipvq_vae_amd  # noqa: F401
    from lipvq_vae_amd import _capi
    from lipvq_vae_amd.tokenizer import _ScreenMonitor
    _ScreenMonitor.ENABLED = False
    print("library:", _capi._LIB_PATH)
    print("EXACT_ROWS = {")
    for (K_, shape_) in sorted(EXACT_ROWS):
        a_, b_, _ = _exact_rows_const(K_, shape_, _capi.set_option)
        assert a_ == b_, (a_, b_)
        print(f"    ({K_}, \"{shape_}\"): {a_},")
    print("}")
