"""GPU: the fused tokenize launch (csrc/lipvq_fused.hip::tokenize_body) at the edges of the instances that the D <= 64 edge files
(test_gpu_tokenize_keepz / _staging / _booking) do not reach.  Inputs: tests/tokenize_cases.py, each shown on the CPU to be the case
it claims to be and to separate a wrong implementation from the right one (tests/test_tokenize_cases_host.py).

Yardstick.  Finite rows: the C oracle (encoder, then `nearest` with the model's rule) and the unfused route (ops.mlp3 with saved
pre-activations + the all-pairs ops.nearest on its z_e): indices, z_e, z_q, usage and the three pre-activations, bit for bit.  A
row whose z_e is not finite has no oracle answer (torch.argmin over NaN is unspecified, csrc/lipvq_screen.hip): it is held to the
unfused route and to the other fused instances of the same model, and it must not change a finite row's answer.  The fast mode is
no parity path: its ring launch is compared with the same launch without the ring, and with parity mode by test_gpu_fast's
near-tie criterion.  No tolerance anywhere else.

Instances <S, FAST, TRAIN, WAVES, COARSE, VQ> reached (tokenize_cases.instance restates tokenize_run / launch_tokenize; each test
asserts the host-side conditions and, where there is one, the observable consequence: `last_exact_rows`, the published list count,
the entry point called):

  A  test_ring_second_lap        <8,0,0,4|8,0,0> and <13,0,0,4,0,0>, in place, caller wants no z_e: the z_e ring, every workgroup-0/1
                                 wave a second row block; against the launch given a z_e buffer (no ring) and tok_inplace = 0
     test_ring_second_lap_fast   <2,1,0,8,0,0> in ring mode against tok_inplace = 0 (the fast entry point takes no z_e buffer: the
                                 list kernel behind a streaming z_e scratch is its launch without a ring)
  B  test_unpacked_bookkeeping   <8,0,0,4|8,0,0> and <8,0,1,8,0,0> under screen_mode = fine: the only PACKF = false instances --
                                 k1[] bookkeeping, pass 3 of lq_screen_decide, emit / in-place decision without keep_mask
  C  test_d208_*, test_fan_in    <13,0,0,4|8,0|1,0>: half-used last tile, streamed layer-2 weights, x_pref on (A <= 16) and off;
                                 the fan-in sweep once at <8,...> too (xq spilled, `k < A` select at load time)
  D  test_one_product_wide       <8|13,0,0,4|8,1,0>, K = 1024 and K = 2049 (ragged last tile, +inf pad tiles, the scanning kernel
                                 behind the list kernel), lists at capacity
  E  test_training_outputs       <2|4|8|13,0,1,8,0|1,0|1>: every output the first N rows of a sentinel-filled allocation
  F  test_vq_*, test_centring_*, <2|8,0,0|1,8,0|1,1>: per-row scales at 2^-20 .. 2^40, dead rows (amax = 0), rows equal to the centring
     test_nonfinite_rows         vector (LLFQ: row_sane false), NaN / inf / 1e30 / 1e37 rows
"""
import numpy as np
import pytest
import torch

from fenced import _Fenced
import tokenize_cases as C

pytestmark = pytest.mark.gpu

A = 7
SHAPES = ["w8rg1", "w4rg1"]
_models = {}
_unfused = {}


def _model(key, variant, p, fan_in, D, K):
    """the module on the GPU with the parameters p; built once per key, never modified"""
    if key not in _models:
        from lipvq_vae_amd.tokenizer import LLFQVAE_V4, VQVAE
        model = (LLFQVAE_V4(fan_in, D, num_codes=K) if variant == "llfq" else VQVAE(fan_in, D, num_embeddings=K)).cuda()
        model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
        assert model.fused_shape()
        _models[key] = model
    return _models[key]


def _fused(model, xt, **kw):
    """one fused launch -> its outputs, the usage it added to zeros, rows decided by an exact stage, the published list count"""
    model.reset_usage()
    out = model._tokenize_fused(xt, model.code_usage, **kw)
    ws = model.last_exact_rows
    head = ws[:2].cpu()
    return dict(idx=out[0], zq=out[1], ze=out[2], pre=out[3] if len(out) > 3 else None, usage=model.code_usage.clone(),
                exact=int(head[0]), listed=int(head[1]))


def _unfused_route(key, model, xt):
    """ops.mlp3 with saved pre-activations + the all-pairs exact kernel on its z_e; once per key"""
    if key not in _unfused:
        from lipvq_vae_amd import ops
        ze, pre = ops.mlp3(xt, model._enc_packed(), model._ENC_ACTS, save_pre=True)
        idx, zq, _ = ops.nearest(ze, model._codebook().detach(), model._DIST)
        _unfused[key] = dict(idx=idx, zq=zq, ze=ze, pre=pre)
    return _unfused[key]


def _same(a, b):
    """a == b everywhere; a NaN equals a NaN (rows that are not finite)"""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _against_references(r, ref, unf, model, N, fin=None):
    """one launch's outputs against the oracle (rows with a finite z_e) and the unfused route (every row)"""
    K = model._codebook().shape[0]
    cb = model._codebook().detach()
    fin = np.ones(N, bool) if fin is None else fin
    idx = r["idx"].cpu().numpy()
    assert np.array_equal(idx[fin], ref["idx"][fin])
    assert int(r["idx"].min()) >= 0 and int(r["idx"].max()) < K
    assert torch.equal(r["zq"], cb[r["idx"]])
    assert np.array_equal(r["zq"].cpu().numpy()[fin], ref["zq"][fin])
    assert int(r["usage"].sum()) == N
    if fin.all():
        assert np.array_equal(r["usage"].cpu().numpy(), ref["usage"])
    assert torch.equal(r["idx"], unf["idx"]) and _same(r["zq"], unf["zq"])
    if r["ze"] is not None:
        assert np.array_equal(r["ze"].cpu().numpy(), ref["ze"], equal_nan=True) and _same(r["ze"], unf["ze"])
    if r["pre"] is not None:
        for got, want, want_u in zip(r["pre"], ref["pre"], unf["pre"]):
            assert np.array_equal(got.cpu().numpy(), want, equal_nan=True) and _same(got, want_u)


def _selected(inst, D, K, **want):
    """the host-side conditions that select the instance a test names"""
    from lipvq_vae_amd import ops
    for k, v in want.items():
        assert inst[k] == v, (k, inst[k], v)
    if not inst["FAST"]:
        assert ops.screen_is_coarse(K, D) == inst["COARSE"]          # (the library's own answer under the options now set)


def _llfq_launches(model, p, x, ref_key, set_option, screen=None, shape=None, train=True, min_exact=0, all_listed=False, fin=None,
                   expect=None):
    """The parity launches of one (model, inputs) pair: the caller wants no z_e (in place where the rule allows: the ring), the same
    launch with tok_inplace = 0, the storing launch (want_ze) and the training launch (want_pre); each against the oracle and the
    unfused route, all with the same indices.  -> the first launch's result"""
    D, K, N = model.latent_dim, model.num_codes, x.shape[0]
    xt = torch.from_numpy(x).cuda()
    ref = C.answers(ref_key, "llfq", p, x)
    unf = _unfused_route(ref_key, model, xt)
    assert _same(unf["ze"], torch.from_numpy(ref["ze"]).cuda())
    runs = [("no z_e", dict(), True), ("no z_e, tok_inplace = 0", dict(), False), ("storing", dict(want_ze=True), True)]
    if train:
        runs.append(("training", dict(want_pre=True), True))
    first = None
    for name, kw, inplace_opt in runs:
        set_option("tok_inplace", "1" if inplace_opt else "0")
        inst = C.instance("llfq", D, K, N, screen=screen, shape=shape, inplace_opt=inplace_opt, **kw)
        want = dict(expect or {})
        if "want_pre" in kw:
            want.update(TRAIN=True, **(dict(WAVES=8) if "WAVES" in want else {}))      # (the training instances have 8 waves only)
        _selected(inst, D, K, **want)
        if name == "no z_e":
            assert D > 64 and inst["ring"] == (not inst["COARSE"] and K <= C.LISTS_ALL_K)
        else:
            assert not inst["ring"]
        r = _fused(model, xt, **kw)
        print(f"{name}: N={N} A={x.shape[1]} D={D} K={K} <S={inst['S']} TRAIN={int(inst['TRAIN'])} WAVES={inst['WAVES']} COARSE={int(inst['COARSE'])}> "
              f"inplace={int(inst['inplace'])} ring={int(inst['ring'])}: exact rows {r['exact']}, listed {r['listed']}")
        _against_references(r, ref, unf, model, N, fin)
        assert r["exact"] >= min_exact, (name, r["exact"], min_exact)
        assert r["listed"] <= r["exact"]                              # (published: rows left to an exact decision >= listed rows)
        if all_listed:
            assert r["exact"] == N and r["listed"] == N
        if first is None:
            first = r
        else:
            assert torch.equal(r["idx"], first["idx"]) and _same(r["zq"], first["zq"]) and torch.equal(r["usage"], first["usage"])
            assert r["exact"] == first["exact"], (name, r["exact"], first["exact"])
    set_option("tok_inplace", "1")
    return first


# ---- A: the z_e ring past its first lap ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,shape", [(128, "w4rg1"), (128, "w8rg1"), (208, "w4rg1")])
def test_ring_second_lap(lipvq_option, no_screen_monitor, D, shape):
    """256 workgroups x one row block, one more full block and a ragged one: the waves of workgroups 0 and 1 store their second
    block's z_e over their first's and decide every row of both in place (every code has a twin one ulp away)."""
    p, x, inst = C.ring_case(D, shape)
    N = x.shape[0]
    model = _model(("ring", D), "llfq", p, A, D, C.RING_K)
    lipvq_option("tok_shape", shape)
    assert inst["ring"] and not inst["KEEPZ"] and inst["WAVES"] == int(shape[1]) and N == inst["lap"] + inst["unit"] + 37
    assert N > C.FUSED_WORKGROUPS * inst["unit"]                      # more row blocks than workgroups
    _llfq_launches(model, p, x, ("ring", D, shape, False), lipvq_option, shape=shape, train=False, min_exact=N, all_listed=True,
                   expect=dict(S=C.screen_S(D), COARSE=False, PACKF=D > 128, WAVES=int(shape[1])))


def test_ring_second_lap_fast(lipvq_option, no_screen_monitor):
    """The fast mode's launch of at most 131 072 rows without a caller's z_e: ring mode.  Same arithmetic with and without the ring."""
    D, K = 32, C.RING_K
    p, x, inst = C.ring_case(D, None, fast=True)
    N = x.shape[0]
    assert inst["ring"] and inst["FAST"] and inst["WAVES"] == 8 and N == 65536 + 256 + 37 <= 131072
    model = _model(("ring", D), "llfq", p, A, D, K)
    xt = torch.from_numpy(x).cuda()
    ring = _fused(model, xt, fast=True)
    lipvq_option("tok_inplace", "0")
    assert not C.instance("llfq", D, K, N, fast=True, inplace_opt=False)["ring"]
    flat = _fused(model, xt, fast=True)
    lipvq_option("tok_inplace", "1")
    print(f"fast, N={N}: exact rows {ring['exact']} (ring), {flat['exact']} (no ring)")
    assert torch.equal(ring["idx"], flat["idx"]) and _same(ring["zq"], flat["zq"]) and torch.equal(ring["usage"], flat["usage"])
    assert ring["exact"] == flat["exact"] == N                        # twins: no row certifiable, whatever its z_e
    cb = model.quantizer.codebook.detach()
    assert torch.equal(ring["zq"], cb[ring["idx"]]) and int(ring["usage"].sum()) == N
    assert int(ring["idx"].min()) >= 0 and int(ring["idx"].max()) < K
    # against parity mode: tests/test_gpu_fast.py's near-tie criterion (the oracle's exact distances from the fp32 z_e)
    ref = C.answers(("ring", D, None, True), "llfq", p, x)
    idx_p = _fused(model, xt)["idx"].cpu().numpy()
    assert np.array_equal(idx_p, ref["idx"])
    idx_f = ring["idx"].cpu().numpy()
    rows = np.flatnonzero(idx_f != idx_p)
    print(f"fast against parity: {rows.size} of {N} indices differ")
    if rows.size:
        d = C.orc().distances(ref["ze"][rows], p[C.CB_KEY["llfq"]])
        dp, df = d[np.arange(rows.size), idx_p[rows]], d[np.arange(rows.size), idx_f[rows]]
        assert np.all(df >= dp)
        assert np.max((df - dp) / dp) <= 5e-3


# ---- B: the unpacked bookkeeping (D = 128 under the three-product screen) ---------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("plant", ["same-lane", "corners", "dup", "upper-half"])
def test_unpacked_bookkeeping(lipvq_option, no_screen_monitor, plant, K, shape):
    """Families (a) - (d) of test_gpu_tokenize_booking.py where the lanes keep k1[] beside m1 / m2: in place, storing, training."""
    D = 128
    p, x = C.planted(plant, A, D, K)
    model = _model(("planted", plant, A, D, K), "llfq", p, A, D, K)
    lipvq_option("screen_mode", "fine")
    lipvq_option("tok_shape", shape)
    floor = {"same-lane": C.N_PLANT, "dup": C.N_PLANT, "corners": 0, "upper-half": x.shape[0]}[plant]
    _llfq_launches(model, p, x, ("planted", plant, A, D, K), lipvq_option, screen="fine", shape=shape, min_exact=floor,
                   all_listed=plant == "upper-half", expect=dict(S=8, COARSE=False, PACKF=False))


# ---- C: D = 208 -------------------------------------------------------------------------------------------------------------------------

WIDE_SCREENS = [(256, "fine"), (1024, "coarse")]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K,screen", WIDE_SCREENS)
@pytest.mark.parametrize("plant", ["corners", "half-tile"])
def test_d208_small_launches(lipvq_option, no_screen_monitor, plant, K, screen, shape):
    """One row, one short of and one past a wave, a ragged second block; the winner in the first / last tile, and codes that differ
    from the winner only in the used half of the last 32-feature tile (the chain's 13th k-step) or only in the first k-step."""
    D = 208
    p, x = C.planted(plant, A, D, K)
    model = _model(("planted", plant, A, D, K), "llfq", p, A, D, K)
    lipvq_option("screen_mode", screen)
    lipvq_option("tok_shape", shape)
    for N in (1, 31, 33, C.N_EDGE):
        _llfq_launches(model, p, x[:N], ("planted", plant, A, D, K, N), lipvq_option, screen=screen, shape=shape,
                       expect=dict(S=13, COARSE=screen == "coarse", PACKF=True, WAVES=int(shape[1])))


FAN_INS = [(208, a) for a in (1, 7, 16, 17, 64)] + [(128, a) for a in (1, 7, 16, 17, 40)]


@pytest.mark.parametrize("K,screen", WIDE_SCREENS)
@pytest.mark.parametrize("D,fan_in", FAN_INS)
def test_fan_in_sweep(lipvq_option, no_screen_monitor, D, fan_in, K, screen):
    """16 | 17: the widest fan-in whose next-block inputs are prefetched and the first that loads them at block start; 64 (D = 128:
    40, see test_fan_in_past_the_lds_budget): the largest supported.  N = 256 + 37: the first block prefetches (or not) the ragged
    second one's rows.  Both workgroup shapes."""
    p = C.params("llfq", fan_in, D, K)
    x = C.inputs(C.X_SEED + 400 + fan_in, C.N_EDGE, fan_in)
    model = _model(("plain", fan_in, D, K), "llfq", p, fan_in, D, K)
    lipvq_option("screen_mode", screen)
    for shape in SHAPES:
        lipvq_option("tok_shape", shape)
        _llfq_launches(model, p, x, ("fan-in", fan_in, D, K), lipvq_option, screen=screen, shape=shape,
                       expect=dict(S=C.screen_S(D), COARSE=screen == "coarse", WAVES=int(shape[1])))


def test_fan_in_past_the_lds_budget(no_screen_monitor):
    """D = 128 keeps layer 2's weights in LDS: beside them layer 0's fragments fit up to a fan-in of 40.  This sweep found
    lipvq_tokenize_supported answering yes up to 64 and the launch then refusing (`168192 B of LDS needed`) -- the module raised
    where it has an unfused route.  Now the query says no, and tokenize() answers through that route, with the oracle's bits."""
    from lipvq_vae_amd import ops
    D, K, fan_in = 128, 256, 64
    assert ops.tokenize_supported(40, 64, 128, D, K) and not ops.tokenize_supported(41, 64, 128, D, K)
    assert not ops.tokenize_supported(fan_in, 64, 128, D, K) and all(ops.tokenize_supported(fan_in, 64, 128, d, K) for d in (32, 64, 208))
    p = C.params("llfq", fan_in, D, K)
    x = C.inputs(C.X_SEED + 400 + fan_in, C.N_EDGE, fan_in)
    from lipvq_vae_amd.tokenizer import LLFQVAE_V4
    model = LLFQVAE_V4(fan_in, D, num_codes=K).cuda()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()})
    assert not model.fused_shape()
    ref = C.answers(("fan-in", fan_in, D, K), "llfq", p, x)
    idx, zq = model.tokenize(torch.from_numpy(x).cuda())
    assert np.array_equal(idx.cpu().numpy(), ref["idx"]) and np.array_equal(zq.cpu().numpy(), ref["zq"])
    assert np.array_equal(model.code_usage.cpu().numpy(), ref["usage"])
    with pytest.raises(Exception, match="unsupported shape"):
        model._tokenize_fused(torch.from_numpy(x).cuda(), None)


# ---- D: the one-product screen at wide latents, both shapes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("plant", ["dup", "upper-half"])
@pytest.mark.parametrize("K", [1024, 2049])
@pytest.mark.parametrize("D", [128, 208])
def test_one_product_wide(lipvq_option, no_screen_monitor, D, K, plant, shape):
    """The default screen of these shapes.  K = 2049: one past LQ_LISTS_ALL_K (the scanning kernel behind the list kernel), a last
    tile of one code (it wins row RAGGED_ROW under `dup`) and +inf pad tiles.  upper-half: every row listed -- the lists at capacity."""
    p, x = C.planted(plant, A, D, K)
    model = _model(("planted", plant, A, D, K), "llfq", p, A, D, K)
    lipvq_option("tok_shape", shape)
    for N in (33, 4 * 32 + 5, C.N_EDGE):
        first = _llfq_launches(model, p, x[:N], ("planted", plant, A, D, K, N), lipvq_option, shape=shape, train=False,
                               min_exact=N if plant == "upper-half" else min(N, C.N_PLANT), all_listed=plant == "upper-half",
                               expect=dict(S=C.screen_S(D), COARSE=True, WAVES=int(shape[1]), inplace=False, ring=False))
        if plant == "dup" and K % 32 and N > C.RAGGED_ROW:
            assert int(first["idx"][C.RAGGED_ROW]) == K - 1


# ---- E: the training instances write their outputs and nothing else ------------------------------------------------------------------------

TRAIN_K = 256


@pytest.mark.parametrize("screen", ["fine", "coarse"])
@pytest.mark.parametrize("D", [32, 64, 128, 208])
@pytest.mark.parametrize("variant", ["llfq", "vq"])
def test_training_outputs_and_nothing_else(monkeypatch, lipvq_option, no_screen_monitor, variant, D, screen):
    """lipvq_tokenize_train_f32 / lipvq_vq_tokenize_train_f32 through the C ABI: idx, z_q, z_e and pre0..2 are the first N rows of
    sentinel-filled allocations, usage starts from a non-zero vector.  N = 1, 31, 33 and 224 + 1: the last waves of the only row
    block hold no (N = 225: one) valid row; 256 + 37: a ragged second block."""
    from lipvq_vae_amd import ops
    K = TRAIN_K
    p = C.params(variant, A, D, K)
    x_all = C.inputs(C.X_SEED + 500 + D, C.N_EDGE, A)
    model = _model(("plain", variant, A, D, K), variant, p, A, D, K)
    lipvq_option("screen_mode", screen)
    cb = model._codebook().detach()
    usage0 = (torch.arange(K, device="cuda", dtype=torch.int64) * 3 + 1)
    entry = "lipvq_tokenize_train_f32" if variant == "llfq" else "lipvq_vq_tokenize_train_f32"
    calls = []
    real = getattr(ops.lib, entry)
    monkeypatch.setattr(ops.lib, entry, lambda *a: (calls.append(1), real(*a))[1])
    for N in (1, 31, 33, 224 + 1, C.N_EDGE):
        x = x_all[:N]
        xt = torch.from_numpy(x).cuda()
        inst = C.instance(variant, D, K, N, screen=screen, want_pre=True)
        _selected(inst, D, K, TRAIN=True, WAVES=8, VQ=variant == "vq", COARSE=screen == "coarse", ring=False, S=C.screen_S(D))
        ref = C.answers(("train", variant, D, N), variant, p, x)
        unf = _unfused_route(("train", variant, D, N), model, xt)
        # through the module's own call first (the entry point the instance belongs to), then on fenced outputs
        n_before = len(calls)
        r = _fused(model, xt, want_pre=True)
        assert len(calls) == n_before + 1
        _against_references(r, ref, unf, model, N)
        f = dict(idx=_Fenced("idx", N, dtype=torch.int64), zq=_Fenced("zq", N, D), ze=_Fenced("ze", N, D), pre0=_Fenced("pre0", N, 64),
                 pre1=_Fenced("pre1", N, 128), pre2=_Fenced("pre2", N, D), usage=_Fenced("usage", K, dtype=torch.int64))
        f["usage"].t.copy_(usage0)
        outs = [f[k].ptr() for k in ("idx", "zq", "usage", "ze", "pre0", "pre1", "pre2")]
        if variant == "llfq":
            packed, raw, _, prep, ws = model._fused_inputs(xt)
            raw_arr = (ops._C.c_void_p * 6)(*[t.data_ptr() for t in raw])
            rc = real(xt.data_ptr(), packed.buf.data_ptr(), raw_arr, cb.data_ptr(), prep.buf.data_ptr(), *outs, ws.data_ptr(),
                      N, A, 64, 128, D, K, ops._stream())
        else:
            packed = model._packed_encoder()
            _, prep, ws = model._fused_operands(xt)
            rc = real(xt.data_ptr(), packed.buf.data_ptr(), cb.data_ptr(), prep.buf.data_ptr(), *outs, ws.data_ptr(),
                      N, A, 64, 128, D, K, ops._stream())
        ops.check(rc, entry)
        torch.cuda.synchronize()
        got = dict(idx=f["idx"].check(), zq=f["zq"].check(), ze=f["ze"].check(), pre=[f[k].check() for k in ("pre0", "pre1", "pre2")],
                   usage=f["usage"].check() - usage0)
        assert int(ws[0]) == r["exact"]
        print(f"{entry} {screen} D={D} N={N}: exact rows {r['exact']}")
        _against_references(got, ref, unf, model, N)


# ---- F: the plain VQVAE's instances ---------------------------------------------------------------------------------------------------------

VQ_SHAPES = [(32, 256, "fine"), (128, 256, "fine"), (32, 1024, "coarse"), (128, 1024, "coarse")]


def _vq_launches(model, p, x, ref_key, D, K, screen, variant="vq", fin=None):
    """the tokenize and the training launch of one (model, inputs) pair against the oracle and the unfused route -> exact rows of both"""
    N = x.shape[0]
    xt = torch.from_numpy(x).cuda()
    ref = C.answers(ref_key, variant, p, x)
    unf = _unfused_route(ref_key, model, xt)
    exact, first = [], None
    for kw in (dict(want_ze=True), dict(want_pre=True)):
        inst = C.instance(variant, D, K, N, screen=screen, **kw)
        _selected(inst, D, K, VQ=variant == "vq", COARSE=screen == "coarse", TRAIN="want_pre" in kw, ring=False, KEEPZ=False,
                  **(dict(WAVES=8) if variant == "vq" else {}))
        r = _fused(model, xt, **kw)
        _against_references(r, ref, unf, model, N, fin)
        assert r["listed"] <= r["exact"]
        exact.append(r["exact"])
        if first is None:
            first = r
        else:
            assert torch.equal(r["idx"], first["idx"]) and _same(r["zq"], first["zq"]) and _same(r["ze"], first["ze"])
    return exact


@pytest.mark.parametrize("D,K,screen", VQ_SHAPES)
def test_vq_scale_sweep(lipvq_option, no_screen_monitor, D, K, screen):
    """W2, b2 and the codebook times 2^e: z_e, the codes and every distance scale exactly, and each row / the codebook carries its
    own power of two into the fp16 fragments -- so the indices are those of e = 0 and the screen certifies the same rows.  All six
    exponents stay inside lq_scale_exp's clamp (k = 13 - floor(log2 max) in [-60, 60]; test_tokenize_cases_host.py asserts it from
    the oracle's z_e), so the count must be the same at every one of them.  None overflows the codebook's fp16 fragments: that
    needs max |2 e'| >= 2^76 past the clamp, where the fp32 distances (2^(2e)) have long overflowed and the oracle defines nothing."""
    lipvq_option("screen_mode", screen)
    p0 = C.params("vq", A, D, K)
    x = C.inputs(C.X_SEED + 60 + D, C.N_EDGE, A)
    idx0 = C.answers(("vq-scale", D, K, 0), "vq", p0, x)["idx"]
    counts = {}
    for e in C.SCALE_EXPONENTS:
        p = C.scaled(p0, e)
        model = _model(("vq-scale", D, K, e), "vq", p, A, D, K)
        counts[e] = _vq_launches(model, p, x, ("vq-scale", D, K, e), D, K, screen)
        assert np.array_equal(C.answers(("vq-scale", D, K, e), "vq", p, x)["idx"], idx0)
    print(f"VQ scale sweep D={D} K={K} {screen}: exact rows (tokenize, training) per exponent {counts}")
    assert len({tuple(v) for v in counts.values()}) == 1, counts


@pytest.mark.parametrize("D,K,screen", VQ_SHAPES)
def test_vq_dead_rows(lipvq_option, no_screen_monitor, D, K, screen):
    """Negative biases: rows of zeros (z_e = 0 exactly, amax of the centred row > 0) beside ordinary rows of the same wave, and a
    launch of nothing but zeros."""
    lipvq_option("screen_mode", screen)
    p = C.dead("vq", C.params("vq", A, D, K))
    model = _model(("vq-dead", D, K), "vq", p, A, D, K)
    for all_zero in (False, True):
        x, rows = C.dead_inputs(A, all_zero)
        exact = _vq_launches(model, p, x, ("vq-dead", D, K, all_zero), D, K, screen)
        print(f"VQ dead rows D={D} K={K} {screen} all_zero={all_zero}: exact rows {exact}")


@pytest.mark.parametrize("screen", ["fine", "coarse"])
@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("variant", ["vq", "llfq"])
def test_rows_equal_to_the_centring_vector(lipvq_option, no_screen_monitor, variant, D, screen):
    """z_e = mu for every row: the centred row is exactly 0 (VQ: amax = 0 takes lq_scale_exp's zero branch; LLFQ: |z'|^2 < tiny2, the
    row is not sane and goes to the exact stage), all 64 distances are equal and the first-index rule answers code 0."""
    lipvq_option("screen_mode", screen)
    K = C.CENTRE_K
    p = C.centred(variant, A, D)
    x = C.inputs(C.X_SEED + 70 + D, C.N_EDGE, A)
    model = _model(("centred", variant, D), variant, p, A, D, K)
    exact = _vq_launches(model, p, x, ("centred", variant, D), D, K, screen, variant=variant)
    print(f"{variant} centring vector D={D} {screen}: exact rows {exact}")
    r = _fused(model, torch.from_numpy(x).cuda(), want_ze=True)
    assert int(r["idx"].max()) == 0 and int(r["usage"][0]) == x.shape[0]
    assert bool((r["ze"] == float(C.CENTRE)).all())
    if variant == "llfq":
        assert exact == [x.shape[0]] * 2                              # row_sane is false for every row


@pytest.mark.parametrize("K,screen", [(256, "fine"), (1024, "coarse")])
@pytest.mark.parametrize("variant", ["vq", "llfq"])
def test_nonfinite_rows(lipvq_option, no_screen_monitor, variant, K, screen):
    """NaN, +-inf, +-1e30 and +-1e37 rows and single elements beside ordinary rows of the same wave, and a wave of nothing else.
    At most the planted rows leave the oracle comparison: those whose z_e, by the oracle, is not finite (the ReLU stack keeps a
    NaN, as torch.relu does, and keeps 1e37 finite: the 1e37 rows stay in; their distances overflow and no code wins: index 0 by
    `v < best`).  A VQ row with a NaN input has a NaN z_e in the torch restatement, in the oracle and (compared with == and NaN
    == NaN in every launch below) in the fused instances, and gets the code of the "no finite distance" rule: 0."""
    D = 128
    lipvq_option("screen_mode", screen)
    p = C.params(variant, A, D, K)
    x, nan_rows, inf_rows, big_rows = C.nonfinite_inputs(A)
    ref = C.answers(("nonfinite", variant, D, K), variant, p, x)
    fin = np.isfinite(ref["ze"]).all(axis=1)
    planted = np.concatenate([nan_rows, inf_rows, big_rows])
    shown = int((~fin)[inf_rows].sum() + (~fin)[big_rows].sum())        # what the oracle's z_e shows for the inf / 1e30 / 1e37 rows
    n_nan = nan_rows.size if variant == "llfq" else int((~fin)[nan_rows].sum())
    assert int((~fin).sum()) == n_nan + shown and np.isin(np.flatnonzero(~fin), planted).all()
    model = _model(("plain", variant, A, D, K), variant, p, A, D, K)
    print(f"{variant} K={K} {screen}: {int((~fin).sum())} of {planted.size} planted rows have a non-finite z_e")
    if variant == "vq":
        restated = C.O.torch_vq_forward({k: torch.from_numpy(np.array(v)) for k, v in p.items()}, torch.from_numpy(x))[2]["z_e"]
        assert bool(restated[nan_rows].isnan().any(1).all()) and bool(np.isnan(ref["ze"][nan_rows]).any(axis=1).all())
        _vq_launches(model, p, x, ("nonfinite", variant, D, K), D, K, screen, fin=fin)
        r = _fused(model, torch.from_numpy(x).cuda(), want_ze=True)
        assert bool(r["ze"][nan_rows].isnan().any(1).all()) and bool((r["idx"][nan_rows] == 0).all())
    else:
        for shape in SHAPES:
            lipvq_option("tok_shape", shape)
            _llfq_launches(model, p, x, ("nonfinite", variant, D, K), lipvq_option, screen=screen, shape=shape, fin=fin,
                           expect=dict(S=8, COARSE=screen == "coarse", WAVES=int(shape[1])))
