"""CPU tests of tests/f16x3_stage_ref.py, the restatement of compute mode f16x3's split kernels that the GPU stage walk
(tests/test_gpu_f16x3_stages.py) holds the device against: its planes represent what tests/test_f16x3_split.py proves they must,
they are cpu_f16x3_emulation.split16's wherever the scales coincide, the launch geometry is the host code's, and every tolerance
of the walk passes a correct (modelled) result while each mutation visible at that stage fails it by at least 10x."""
import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests import f16x3_stage_ref as R
from tests.cpu_f16x3_emulation import split16


def _problem(N=2304, D=5, S=8, M=120, abc=(-1.0, 0.0, -1.0), seed=0x5CF6F200):
    X = synth.make_X(seed, N, D)
    y = synth.normal(seed + 1, 0, N)
    p = synth.make_params(seed + 2, D, S, M, abc=abc)
    Phi = O.feature_map(X, p, D, S, M)
    K = Phi.shape[1]
    Phi32 = Phi.astype(np.float32)
    P = Phi32.astype(np.float64)
    B = np.linalg.inv(P.T @ P + (np.exp(2 * p[0]) + 1e-6) * np.eye(K))
    s = np.exp(p[1]) * np.sqrt(2.0 / M)
    return Phi32, y, B, s, p, K, M


def test_planes_encode_and_decode_round_trip():
    rng = np.random.default_rng(1)
    h = rng.standard_normal((7, 64)).astype(np.float16); l = (rng.standard_normal((7, 64)) * 1e-3).astype(np.float16)
    w = R.encode_planes(h, l)
    assert w.dtype == np.uint32 and w.shape == (7, 64)
    # the layout: per 16 columns 16 h's (32 bytes), then 16 l's
    assert np.array_equal(w[0, :8].view(np.float16), h[0, :16]) and np.array_equal(w[0, 8:16].view(np.float16), l[0, :16])
    h2, l2 = R.decode_planes(w)
    assert np.array_equal(h2.view(np.uint16), h.view(np.uint16)) and np.array_equal(l2.view(np.uint16), l.view(np.uint16))


@pytest.mark.parametrize('b', [-6.0, 0.0, 6.0])
def test_emulated_planes_represent_their_values_as_the_split_tests_prove(b):
    Phi32, y, B, s, p, K, M = _problem(abc=(-1.0, b, -1.0))
    h, l, e = R.split_rows(Phi32, np.float32(s))
    assert e == R.exponent(s) and 2.0 ** 14 <= float(np.float32(s)) * 2.0 ** e < 2.0 ** 15
    x = Phi32.astype(np.float64)
    back = R.planes_value(h, l, e)
    assert np.all(np.abs(back - x) <= 2.0 ** -22.9 * np.abs(x) + 2.0 ** -25 * 2.0 ** -e)
    assert np.all(np.abs(back - x) <= 2.0 ** (-9 - e))                # half a step of l below 2^15, scaled back
    # the weighted planes (qV16g): q o V to the same relative accuracy, against the bound of |q V|
    V32 = (x @ B).astype(np.float32)
    q = np.abs(synth.normal(7, 0, V32.shape[0])) * 0.3
    q[5] = 40.0                                                 # one row whose q is far above the rest
    vb = R.v_bound(B, K, s, M)
    maxq = np.float32(np.abs(q).max() * (1 + 1e-6))
    assert np.abs(V32).max() <= vb
    hq, lq, e1 = R.split_rows_weighted(V32, q, vb, maxq)
    f = (q * 2.0 ** e1).astype(np.float32)
    qv = (V32 * f[:, None]).astype(np.float64) * 2.0 ** -e1              # the kernel splits x f rounded to fp32
    back = R.planes_value(hq, lq, e1)
    assert np.all(np.abs(back - qv) <= 2.0 ** -22.9 * np.abs(qv) + 2.0 ** -25 * 2.0 ** -e1)
    assert np.all(np.isfinite(hq)) and np.all(np.isfinite(lq))


def test_emulated_planes_are_split16_where_the_scales_coincide():
    Phi32, y, B, s, p, K, M = _problem()
    h, l, e = R.split_rows(Phi32, np.float32(s))
    h0, l0, e0 = split16(Phi32.astype(np.float64))
    assert e == e0                                               # max |Phi| and s share their binade here
    assert np.array_equal(h.astype(np.float32), h0) and np.array_equal(l.astype(np.float32), l0)
    hB, lB, s0, s1 = R.split_operand(B, K, s)
    bh, bl, eb = split16(B)
    assert s1 == 2.0 ** eb and s0 == 2.0 ** -(eb + e)
    assert np.array_equal(hB[:K, :K].astype(np.float32), bh.T) and np.array_equal(lB[:K, :K].astype(np.float32), bl.T)


def test_the_low_half_against_a_different_h_is_a_step_of_h_off():
    """the weighted split as the compiler once made it (R.split_rows_weighted model 'mix': l formed against h' = fp16(x f) rounded
    once from the exact product, h = fp16(fp32(x f)) stored) differs from the kernel's own rule on some elements, and there h + l is
    off by a step of h, 2^-11 of the value, where the rule keeps 2^-22"""
    rng = np.random.default_rng(3)
    V = rng.standard_normal((4096, 64)).astype(np.float32)
    q = rng.uniform(0.1, 3.0, 4096)
    a = R.split_rows_weighted(V, q, np.abs(V).max() * 1.01, q.max() * 1.01)
    b = R.split_rows_weighted(V, q, np.abs(V).max() * 1.01, q.max() * 1.01, model='mix')
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    xf = (V * (q * 2.0 ** a[2]).astype(np.float32)[:, None]).astype(np.float64)
    da = np.abs(R.planes_value(a[0], a[1], 0) - xf); db = np.abs(R.planes_value(b[0], b[1], 0) - xf)      # scaled units
    assert np.all(da <= 2.0 ** -22.9 * np.abs(xf) + 2.0 ** -25)
    off = db > 2.0 ** -14 * np.abs(xf)
    assert 0 < off.sum() < 1e-3 * off.size and np.all(db[off] >= 2.0 ** -12 * np.abs(xf[off]))


def test_launch_geometry_restated_from_the_host_code():
    assert R.apply_plan(132) == (0, 0, 3)                       # K <= 256: no 128-wide blocks, so no f16 apply tiles
    assert not R.f16_apply_runs(256) and R.f16_apply_runs(257)
    assert R.apply_plan(2112) == (16, 2048, 1)
    pl = R.f16_apply_tiles(2112, 33 * 256, 256)                 # 33 row blocks x 8 = 264 tiles on 256 CUs: 8 in the last round
    assert pl['n256'] == 8 and pl['tail_rb'] == 1
    assert R.f16_apply_tiles(2112, 32 * 256, 256)['tail_rb'] == 0
    assert [w for _, w in R.f16_apply_tiles(640, 2304, 256)['main']] == [256, 256, 128]
    assert [w for _, w in R.f16_apply_tiles(4224, 2048, 256)['main']].count(128) == 1
    assert R.gram_tiles(640) == 11 and R.gram_tiles(4224) == 2 * (16 * 17 // 2) + 33          # 256-blocks 0..15 and the 17th, sticking out
    assert R.f16_chunk(71936, 640, 640) == 1280 and R.gram_chunks(71936, 1280) == (1280, 57, 256)
    assert R.f16_chunk(2304, 640) == 1024 and R.gram_chunks(2304, 1024) == (1024, 3, 256)


# ---- the tolerances' teeth ---------------------------------------------------------------------------------------------------
def _gram_fig(G, G3, absn, K):
    return R.worst(R.tile_errors(R.normalised(G, G3, absn), K))[0]


def _apply_fig(V, V3, absn, N, K):
    return R.worst(R.apply_errors(R.normalised(V, V3, absn), N, K))[0]


def test_gram_tolerance_passes_the_model_and_fails_every_visible_mutation_tenfold():
    Phi32, y, B, s, p, K, M = _problem()
    N = Phi32.shape[0]
    h, l, e = R.split_rows(Phi32, np.float32(s))
    sc = 2.0 ** (-2 * e)
    G3 = R.gram3(h, l, h, l, sc)
    absn = np.abs(Phi32.astype(np.float64)).T @ np.abs(Phi32.astype(np.float64))
    chunk = 1024                                                # 2304 rows: chunks of 1024, 1024 and a short last one of 256
    model = R.gram_device_model(h, l, h, l, sc, chunk)
    ok = _gram_fig(model, G3, absn, K)
    assert ok <= R.CAP_GRAM3 / 10, ok                           # a correct result passes, with room
    z = np.zeros_like(h)
    hz = h.copy(); lz = l.copy(); hz[256:512] = 0; lz[256:512] = 0
    tile = model.copy(); tile[128:256, 0:128] = model[128:256, 128:256]
    mutants = {
        'drop Al.Bh': R.gram_device_model(h, z, h, l, sc, chunk),         # the A side loses its l's, Ah.Bl stays
        'drop Ah.Bl': R.gram_device_model(h, l, h, z, sc, chunk),
        'h only': R.gram_device_model(h, z, h, z, sc, chunk),
        'exponent off by one': model * 2,
        'a 128-tile from its neighbour': tile,
        'a 256-row block zeroed': R.gram_device_model(hz, lz, hz, lz, sc, chunk),
        'the last short chunk dropped': R.gram_device_model(h[:2048], l[:2048], h[:2048], l[:2048], sc, chunk),
    }
    for nm, G in mutants.items():
        f = _gram_fig(G, G3, absn, K)
        assert f >= 10 * R.CAP_GRAM3, (nm, f)
    # two rows swapped across a fold boundary: a Gram of ONE operand is a sum over its rows, which no order changes -- invisible at
    # pass 1's Gram by construction; the weighted Gram and V = Phi B see it (below)
    hs = h.copy(); ls = l.copy(); hs[[511, 512]] = hs[[512, 511]]; ls[[511, 512]] = ls[[512, 511]]
    assert _gram_fig(R.gram_device_model(hs, ls, hs, ls, sc, chunk), G3, absn, K) <= R.CAP_GRAM3


def test_weighted_gram_tolerance_sees_V16g_left_at_zero_and_swapped_rows():
    Phi32, y, B, s, p, K, M = _problem()
    N = Phi32.shape[0]
    V32 = (Phi32.astype(np.float64) @ B).astype(np.float32)
    q = 0.2 + np.abs(synth.normal(11, 0, N))
    vb = R.v_bound(B, K, s, M); maxq = np.float32(q.max() * (1 + 1e-6))
    hv, lv, ev = R.split_rows(V32, vb)
    hq, lq, eq = R.split_rows_weighted(V32, q, vb, maxq)
    sc = 2.0 ** -(ev + eq)
    W3 = R.gram3(hv, lv, hq, lq, sc)
    Vd = V32.astype(np.float64)
    absn = np.abs(Vd).T @ (q[:, None] * np.abs(Vd))
    model = R.gram_device_model(hv, lv, hq, lq, sc, 1024)
    assert _gram_fig(model, W3, absn, K) <= R.CAP_GRAM3 / 10
    z = np.zeros_like(hv)
    assert _gram_fig(R.gram_device_model(z, z, hq, lq, sc, 1024), W3, absn, K) >= 10 * R.CAP_GRAM3        # V16g left at zero
    hs = hv.copy(); ls = lv.copy(); hs[[511, 512]] = hs[[512, 511]]; ls[[511, 512]] = ls[[512, 511]]
    assert _gram_fig(R.gram_device_model(hs, ls, hq, lq, sc, 1024), W3, absn, K) >= 10 * R.CAP_GRAM3        # one operand's rows swapped
    assert _gram_fig(model * 2, W3, absn, K) >= 10 * R.CAP_GRAM3


def test_apply_tolerance_passes_the_model_and_fails_every_mutation_tenfold():
    Phi32, y, B, s, p, K, M = _problem()
    N = Phi32.shape[0]
    h, l, e = R.split_rows(Phi32, np.float32(s))
    hB, lB, s0, s1 = R.split_operand(B, K, s)
    V3 = R.apply3(h, l, hB, lB, s0)
    absn = np.abs(Phi32.astype(np.float64)) @ np.abs(B)
    model = R.apply_device_model(h, l, hB, lB, s0)
    ok = _apply_fig(model, V3, absn, N, K)
    assert ok <= R.CAP_APPLY3 / 10, ok
    z = np.zeros_like(hB); zp = np.zeros_like(h)
    tile = model.copy(); tile[:, 128:256] = model[:, 0:128]
    rows = model.copy(); rows[256:512] = 0
    sw = model.copy(); sw[[511, 512]] = sw[[512, 511]]
    short = model.copy(); short[2048:] = 0
    mutants = {
        'drop Al.Bh': R.apply_device_model(h, zp, hB, lB, s0),
        'drop Ah.Bl': R.apply_device_model(h, l, hB, z, s0),
        'h only': R.apply_device_model(h, zp, hB, z, s0),
        'exponent off by one': model * 2,
        'a column tile from its neighbour': tile,
        'a 256-row block zeroed': rows,
        'two rows swapped across a 512-row fold': sw,
        'the last short row block dropped': short,
    }
    for nm, V in mutants.items():
        f = _apply_fig(V, V3, absn, N, K)
        assert f >= 10 * R.CAP_APPLY3, (nm, f)


def test_the_4x_rule_floor_is_below_what_a_dropped_term_costs():
    """the walk's comparisons against the exact fp32 product allow 4x the fp32 context's error plus FLOOR_SPLIT; a term dropped from
    the split (2^-11 of the operands, element for element) must stand out of that floor by 10x on a product over the columns"""
    Phi32, y, B, s, p, K, M = _problem()
    N = Phi32.shape[0]
    h, l, e = R.split_rows(Phi32, np.float32(s))
    hB, lB, s0, s1 = R.split_operand(B, K, s)
    P = Phi32.astype(np.float64)
    Vx = P @ B.astype(np.float32).astype(np.float64)
    absn = np.abs(P) @ np.abs(B)
    zp = np.zeros_like(h)
    assert _apply_fig(R.apply_device_model(h, l, hB, lB, s0), P @ B, absn, N, K) <= R.FLOOR_SPLIT
    assert _apply_fig(R.apply_device_model(h, zp, hB, lB, s0), P @ B, absn, N, K) >= 10 * R.FLOOR_SPLIT
    assert _apply_fig(R.apply_device_model(h, zp, hB, np.zeros_like(hB), s0), Vx, absn, N, K) >= 10 * R.FLOOR_SPLIT


def test_outlier_rule_catches_one_bad_block():
    rng = np.random.default_rng(5)
    blocks = {(i, 0): float(v) for i, v in enumerate(rng.uniform(1e-8, 3e-8, 40))}
    assert not R.outliers(blocks, R.CAP_GRAM3)
    blocks[(17, 0)] = 5e-7
    assert list(R.outliers(blocks, R.CAP_GRAM3)) == [(17, 0)]
