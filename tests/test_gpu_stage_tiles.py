"""
fp64 and fp32 mode stage by stage, per tile: an engine walks pass1 -> factor -> pass2 -> adjoint -> pass3 -> finish, and every stage
is compared with an fp64 numpy restatement computed from that engine's own inputs to the stage (read back with debug_read), so that
each bound measures that kernel's error alone, not the conditioning upstream.  Products are held to the normalised error
|X - X_ref| / (|A|^T |B|), worst per tile of the kernel's own tiling (128-tiles and the 64-strip of the Gram, column tiles of the
apply launch plan x 256-row blocks), against a-priori bounds (tests/parity.py: bound32 / bound64), never fitted ones.  The K-stage
is held to c K u64 cond(A) with cond of the engine's own A = G + lambda I.  The end-to-end result meets the oracle through
tests/parity.py's block checks.  Each shape asserts the path it is for (launch geometry restated from the host code).
"""
import numpy as np
import pytest
import torch

from oracle import scfgp_oracle as O
from tests import parity as P
from tests import f16x3_stage_ref as R
from tests.golden.make_oracle_kats import CASES, case_inputs

pytestmark = pytest.mark.gpu

C_KSTAGE = 1.0              # c of the K-stage bounds c K u64 cond(A)

# id -> (D, S, M, N, options, dtypes); None for N: a KAT case
SHAPES = {
    'tiny_257x5': (None, None, None, None, {}, ('f64', 'f32')),
    'kin8nm_like': (None, None, None, None, {}, ('f64', 'f32')),
    'c1_boston_shape': (None, None, None, None, {}, ('f64', 'f32')),
    'k320_n9001': (6, 20, 140, 9001, {}, ('f64', 'f32')),
    'k544_dma0': (16, 16, 256, 6000, {'apply_dma': 0}, ('f64', 'f32')),
    'k544_dma1': (16, 16, 256, 6000, {'apply_dma': 1}, ('f64', 'f32')),
    'k544_dma2': (16, 16, 256, 6000, {'apply_dma': 2}, ('f32',)),
    'k640_n5000': (8, 20, 300, 5000, {}, ('f64', 'f32')),
    'k704_n5000': (8, 32, 320, 5000, {}, ('f64', 'f32')),
    'k2112_rankS': (64, 32, 1024, 9000, {'lowrank_bwd': 1}, ('f64', 'f32')),
    'k320_level1': (6, 20, 140, 9001, {'gram64': 1}, ('f32',)),
    'k320_level2': (6, 20, 140, 9001, {'gram64': 3}, ('f32',)),
}
CASE_IDS = [(n, dt) for n, v in SHAPES.items() for dt in v[5]]


def _inputs(name):
    D, S, M, N, opts, _ = SHAPES[name]
    if N is None:
        N, D, S, M, T, seed = CASES[name]
        X, y, params, Xs = case_inputs(name)
        return D, S, M, N, X, y, params
    from scfgp_amd import synth
    seed = 0x5CF6E000 + 7 * M + N
    X = synth.make_X(seed, N, D)
    y = synth.normal(seed + 1, 0, N).reshape(-1, 1)
    params = synth.make_params(seed + 2, D, S, M, abc=(-1.0, 0.0, -1.0))
    return D, S, M, N, X, y, params


def _apply_tiles(K, Np, dma):
    """column tiles of the apply launch: 256-wide with apply_dma = 2 (where K > 256), else apply.hip's 128 + 64 plan"""
    if dma == 2 and R.f16_apply_runs(K):
        return R.f16_apply_tiles(K, Np, torch.cuda.get_device_properties(0).multi_processor_count)['main']
    c128, col64, c64 = R.apply_plan(K)
    return [(128 * i, 128) for i in range(c128)] + [(col64 + 64 * i, 64) for i in range(c64)]


def _reach(name, K, Kp, Np, N, eng, dtype):
    """the path the shape is for"""
    if name in ('tiny_257x5', 'kin8nm_like', 'c1_boston_shape'):
        assert K <= 256 and R.apply_plan(K)[0] == 0 and R.apply_plan(K)[2] <= 4      # one 64-wide launch
    if name.startswith('k320'):
        assert K == 320 and Kp == 384 and R.apply_plan(K) == (2, 256, 1) and Np % 256 == 0 and N % 256 != 0
        assert -(-N // 4096) == 3                                                       # three chains of the 4096-row flush
    if name.startswith('k544'):
        assert K == 544 and R.apply_plan(K) == (4, 512, 1)
    if name.startswith('k640'):
        assert K == 640 and Kp // 128 == 5                                              # unpaired last block row
    if name.startswith('k704'):
        assert K == 704 and Kp == 768 and Kp // 128 == 6 and K % 128 == 64              # 64-column strip
    if name == 'k2112_rankS':
        assert K == 2112 and Kp == 2176
    lvl = eng.condition()['level'] if dtype == 'f32' else 0
    want = {'k320_level1': 1, 'k320_level2': 2}.get(name, 0)
    assert lvl == want, (name, lvl)


def _tiles_gram(err, K):
    e = P.edges(K, 128)
    return P.stage_error(err[0], err[1], err[2], e, e).max()


def _tiles_apply(X, Xr, sc, N, K, tiles):
    re = P.edges(N, 256)
    ce = sorted(set([c for c, w in tiles if c < K] + [K]))
    return P.stage_error(X, Xr, sc, re, ce).max()


@pytest.mark.parametrize('name,dtype', CASE_IDS, ids=['%s-%s' % c for c in CASE_IDS])
def test_stage_tiles(name, dtype):
    from scfgp_amd.engine import HipEngine
    D, S, M, N, X, y, params = _inputs(name)
    opts = dict(SHAPES[name][4])
    J = S + M; K = 2 * J
    yv = y.ravel()
    e = HipEngine(D, S, M, dtype=dtype)
    if dtype == 'f32':
        e.set_option('gram64', opts.pop('gram64', 0))
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_params(params); e.set_data(X, y)
    e.set_profiling(True)
    d = e.dims(); Kp, Jp, Dp, Np = d['Kp'], d['Jp'], d['Dp'], d['Np']
    f32 = dtype == 'f32'
    tdt = np.float32 if f32 else np.float64
    dma = SHAPES[name][4].get('apply_dma', 1 if K > 256 else 0)
    tiles = _apply_tiles(K, Np, dma)
    figs = []                                                # (stage, worst, bound)

    def fig(stage, worst, bound):
        figs.append((stage, float(worst), float(bound)))
        print('%s %s %-28s worst %.2e  bound %.2e  (%.2gx below)' % (name, dtype, stage, worst, bound, bound / max(worst, 1e-300)),
              flush=True)

    # ---- pass 1: G = Phi^T Phi, Phi^T y
    e.pass1()
    level = {1: 1, 3: 2}.get(SHAPES[name][4].get('gram64', 0), 0)
    Phi = e.debug_read('Phi', (Np, Kp), tdt).astype(np.float64)
    P64 = Phi[:N, :K]; absP = np.abs(P64)
    if level:
        Pg = e.debug_read('Phi64', (Np, Kp))[:N, :K]           # the escalated pass 1's Gram runs on fp64 features
        assert np.linalg.norm(Pg - P64) <= 1e-6 * np.linalg.norm(Pg)
    else:
        Pg = P64
    x1 = e.debug_read('G', (Kp * Kp + Kp + 8,))
    G = x1[:Kp * Kp].reshape(Kp, Kp)[:K, :K]; gy = x1[Kp * Kp:Kp * Kp + K]
    fp64_gram = not f32 or SHAPES[name][4].get('gram64', 0) > 0
    bG = P.bound64(N) if fp64_gram else P.bound32(4096, n64=Np // 64)
    fig('G per 128-tile', _tiles_gram((G, Pg.T @ Pg, np.abs(Pg).T @ np.abs(Pg)), K), bG)
    bgy = P.bound64(N) if fp64_gram else P.bound32(4096, n64=Np // 64, rounded=1)
    fig('Phi^T y per 128-block', (np.abs(gy - Pg.T @ yv) / (np.abs(Pg).T @ np.abs(yv))).max(), bgy)

    # ---- factor
    assert e.factor()
    Li = e.debug_read('Li', (Kp, Kp))[:K, :K]; B = e.debug_read('B', (Kp, Kp))[:K, :K]
    vecs1 = e.debug_read('vecs', (5, Kp)); al = vecs1[1, :K]
    lam = np.exp(2 * params[0]) + O.EPSILON
    A = G + lam * np.eye(K)
    cA = np.linalg.cond(A)
    bK = C_KSTAGE * K * P.U64 * cA
    fig('Li A Li^T - I (max)', np.abs(Li @ A @ Li.T - np.eye(K)).max(), bK)
    a_ref = np.linalg.solve(A, gy)
    fig('alpha per 64-tile', max(np.linalg.norm(al[i:i + 64] - a_ref[i:i + 64]) / np.linalg.norm(a_ref) for i in range(0, K, 64)), bK)
    B_ref = Li.T @ Li
    fig('B per 64-tile', P.stage_error(B, B_ref, np.abs(Li).T @ np.abs(Li), P.edges(K, 64), P.edges(K, 64)).max(), P.bound64(K))

    # ---- pass 2: V = Phi B (or C = Phi Li^T, V = C Li), p, q, the weighted Gram
    e.pass2(True)
    V = e.debug_read('V', (Np, Kp), tdt).astype(np.float64)[:N, :K]
    p = e.debug_read('p', (Np,))[:N]; q = e.debug_read('q', (Np,))[:N]
    x2 = e.debug_read('W', (Kp * Kp + Kp + 8,))
    W = x2[:Kp * Kp].reshape(Kp, Kp)[:K, :K]; wp = x2[Kp * Kp:Kp * Kp + K]
    bA = P.bound32(K, rounded=1, out32=True) if f32 else P.bound64(K)
    cform = level == 2
    if cform:
        Cm = e.debug_read('C', (Np, Kp), tdt).astype(np.float64)[:N, :K]
        fig('C = Phi Li^T per tile', _tiles_apply(Cm, P64 @ Li.T, absP @ np.abs(Li.T), N, K, tiles), bA)
        fig('V = C Li per tile', _tiles_apply(V, Cm @ Li, np.abs(Cm) @ np.abs(Li), N, K, tiles), bA)
        Mw = Cm
    else:
        fig('V = Phi B per tile', _tiles_apply(V, P64 @ B, absP @ np.abs(B), N, K, tiles), bA)
        Mw = V
    kappa = np.log1p(np.exp(params[2]))
    Vs = P64 @ B if cform else V                              # v = sum V o Phi of the engine's operands
    mu = P64 @ al; mabs = absP @ np.abs(al)
    v = (Vs * P64).sum(1)
    vabs = ((absP @ np.abs(Li.T)) ** 2).sum(1) if cform else (np.abs(Vs) * absP).sum(1)
    dd = kappa * (v + 1); r = mu - yv
    ee = 1 / dd - (r * r + v) / dd ** 2
    px = 2 * r / dd; qx = 1 / dd + kappa * ee
    pabs = 2 / dd * mabs + 2 * np.abs(r) * kappa / dd ** 2 * vabs
    qabs = 2 * kappa * np.abs(r) / dd ** 2 * mabs + ((1 + 2 * kappa) * kappa / dd ** 2 + 2 * kappa ** 2 * (r * r + np.abs(v)) / dd ** 3) * vabs
    bpq = (P.bound32(K + 2, rounded=1, out32=True) if f32 else P.bound64(K + 4))
    if cform:
        bpq = 2 * bA                                          # v from C's rows: the factor form's own rounding enters twice
    fig('p elementwise', (np.abs(p - px) / pabs).max(), bpq)
    fig('q elementwise', (np.abs(q - qx) / qabs).max(), bpq)
    Mabs = np.abs(Mw)
    bW = P.bound64(N) if not f32 else P.bound32(4096, n64=Np // 64, rounded=2)
    fig('W per 128-tile', _tiles_gram((W, Mw.T @ (q[:, None] * Mw), Mabs.T @ (np.abs(q)[:, None] * Mabs)), K), bW)
    # the exchanged matrix is symmetric to within its two triangles' own errors (each within bW of the exact product)
    Wa = Mabs.T @ (np.abs(q)[:, None] * Mabs)
    fig('W - W^T (diagonal 128-tiles)', (np.abs(W - W.T) / Wa).max(), 2 * bW)
    fig('side (V^T p) per 128-block', (np.abs(wp - Mw.T @ p) / (Mabs.T @ np.abs(p))).max(), bW)

    # ---- adjoint: Abar from the engine's B, the exchanged B W B (or C^T q C turned into it) and u
    e.adjoint()
    Abar = e.debug_read('Abar', (Kp, Kp))[:K, :K]; vecs = e.debug_read('vecs', (5, Kp)); ut = vecs[3, :K]
    em2a = np.exp(-2 * params[0])
    if cform:
        # kstage_adjoint_factor_form: T1 = Mc Li with Mc read as stored [k][m] (i.e. Mc^T), then Li^T T1 on the lower 64-tiles,
        # each mirrored into the upper one.  Mc = the exchanged C^T q C is symmetric only to the fp32 Gram's rounding (both
        # triangles of a diagonal 128-tile are accumulated separately, checked above), so the restatement reads it the same way
        t64 = np.arange(K) // 64
        X2 = Li.T @ W.T @ Li; X2a = np.abs(Li).T @ np.abs(W) @ np.abs(Li)
        low = t64[:, None] >= t64[None, :]
        BWB = np.where(low, X2, X2.T); BWBa = np.where(low, X2a, X2a.T); u = Li.T @ wp
        ua = np.abs(Li).T @ np.abs(wp); bAb = P.bound64(2 * K + 8)
    else:
        BWB, BWBa, u, ua, bAb = W, np.abs(W), wp, np.abs(wp), P.bound64(8)
    Ab_ref = B - BWB - 0.5 * (np.outer(u, al) + np.outer(al, u)) + em2a * np.outer(al, al)
    Ab_abs = np.abs(B) + BWBa + 0.5 * (np.outer(ua, np.abs(al)) + np.outer(np.abs(al), ua)) + em2a * np.outer(np.abs(al), np.abs(al))
    fig('Abar per 64-tile', P.stage_error(Abar, Ab_ref, Ab_abs, P.edges(K, 64), P.edges(K, 64)).max(), bAb)

    # ---- pass 3: Phibar, then X~^T Zbar (or the rank-S form's T~^T Zbar and X~^T U)
    e.pass3()
    Pb = e.debug_read('V', (Np, Kp), tdt).astype(np.float64)[:N]
    Xt = e.debug_read('Xt', (Np, Dp))[:N]
    lrb = SHAPES[name][4].get('lowrank_bwd', -1) == 1
    if lrb:                                                  # host code: want_lrb() -- the projection through S, U fits in Phibar
        assert -(-(S + 1) // 16) * 16 < Dp and Jp + -(-S // 64) * 64 <= Kp
    Dpp = -(-Dp // 128) * 128
    if lrb:
        Sp = -(-(S + 1) // 16) * 16; Spp = -(-Sp // 128) * 128; Sq = -(-S // 128) * 128
        x3 = e.debug_read('XZ', (max(Dpp, Spp) * Jp + 8 + Dpp * Sq,))
        TZ = x3[:Spp * Jp].reshape(Spp, Jp); XU = x3[Dpp * Jp + 8:].reshape(Dpp, Sq)
        Tt = e.debug_read('Tt', (Np, Sp))[:N]
        Zb = Pb[:, :J]; U = Pb[:, Jp:Jp + S]
        rF = params[3 + D * S:3 + D * S + M * S].reshape(M, S)
        bU = P.bound32(M, rounded=1, out32=True) if f32 else P.bound64(M + 1)
        fig('U = Zbar_L + Zbar_M r_F per tile', _tiles_apply(U, Zb[:, :S] + Zb[:, S:] @ rF,
                                                              np.abs(Zb[:, :S]) + np.abs(Zb[:, S:]) @ np.abs(rF), N, S, [(0, 64)]), bU)
        bT = P.bound32(4096, n64=Np // 64, rounded=1) if f32 else P.bound64(N)
        e_tz = P.stage_error(TZ[:S + 1, :J], Tt[:, :S + 1].T @ Zb, np.abs(Tt[:, :S + 1]).T @ np.abs(Zb), P.edges(S + 1, 128), P.edges(J, 128))
        fig('T~^T Zbar per 128-tile', e_tz.max(), bT)
        assert np.allclose(Tt[:, S], 1.0)                     # T~'s ones column: the phase sums
        e_xu = P.stage_error(XU[:D + 1, :S], Xt[:, :D + 1].T @ U, np.abs(Xt[:, :D + 1]).T @ np.abs(U), P.edges(D + 1, 128), P.edges(S, 128))
        fig('X~^T U per 128-tile', e_xu.max(), bT)
        ones = (np.abs(TZ[S, :J] - Zb.sum(0)) / np.abs(Zb).sum(0)).max()
        fig('ones row (phase sums)', ones, bT)
    else:
        Pb = Pb[:, :K]
        rest = np.outer(p, al) + np.outer(yv, ut) + 2 * q[:, None] * Vs
        rabs = np.abs(np.outer(p, al)) + np.abs(np.outer(yv, ut)) + 2 * np.abs(q[:, None] * Vs)
        if not cform:
            bP = P.bound32(K + 4, rounded=2, out32=True) if f32 else P.bound64(K + 4)
            fig('Phibar per tile', _tiles_apply(Pb, rest + 2 * P64 @ Abar, rabs + 2 * absP @ np.abs(Abar), N, K, tiles), bP)
        x3 = e.debug_read('XZ', (Dpp * Jp + 8,))
        XZ = x3[:Dpp * Jp].reshape(Dpp, Jp)
        Zc = P64[:, :J] * Pb[:, J:]; Zs = P64[:, J:] * Pb[:, :J]
        Zb = Zc - Zs; Za = np.abs(Zc) + np.abs(Zs)
        bX = P.bound32(4096 + 2, n64=Np // 64, rounded=1) if f32 else P.bound64(N + 3)
        fig('X~^T Zbar per 128-tile', P.stage_error(XZ[:D + 1, :J], Xt[:, :D + 1].T @ Zb, np.abs(Xt[:, :D + 1]).T @ Za,
                                                    P.edges(D + 1, 128), P.edges(J, 128)).max(), bX)
        assert np.allclose(Xt[:, D], 1.0)
        fig('ones row (phase sums)', (np.abs(XZ[D, :J] - Zb.sum(0)) / Za.sum(0)).max(), bX)

    # ---- finish, against the oracle per block
    res = e.finish(True)
    _reach(name, K, Kp, Np, N, e, dtype)
    ref = P.oracle_all(X, y, params, S, M)
    ratios = P.grad_ratios(res[1], ref['grad'], ref['scale'], D, S, M, dtype)
    ratios['alpha'] = P.alpha_ratio(res[2], ref['alpha'], dtype); ratios['Li'] = P.li_ratio(res[3], ref['Li'], dtype)
    print('%s %s end to end (ratio to the %s row): %s' % (name, dtype, dtype, P.fmt(ratios)), flush=True)
    e.close()
    bad = [f for f in figs if not f[1] <= f[2]]
    assert not bad, bad
    assert max(ratios.values()) <= 1.0, ratios
