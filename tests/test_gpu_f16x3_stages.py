"""
Compute mode f16x3 stage by stage: the split kernels' own outputs (the plane arrays, bounds and scales, through debug_read) against
their bit-exact CPU restatement (tests/f16x3_stage_ref.py), each product against its exact three-term value from the planes, and
every stage against the exact product of its fp32 operands under the 4x rule of fp32 mode's tier -- per 128-tile, per column tile
of the apply launch plan and per 256-row block, so that one bad tile, tail row block or chunk cannot hide under a norm over the
whole matrix.  The shapes reach the paths their names give, and each test asserts that it does (launch geometry restated from the
host code).  An fp32 context with the same options and data walks beside the f16x3 one: its error on the same block is the yardstick.
"""
import sys

import numpy as np
import pytest
import torch

from tests import f16x3_stage_ref as R

pytestmark = pytest.mark.gpu

D = 6


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _n_for_tail(ncu):
    """rows for K = 2112 (8 x 256 + 64 columns) whose 256-wide tiles leave a last round < 0.45 full, so that tail_rb >= 1"""
    for nrb in range(ncu // 8 + 1, 4 * ncu):
        if R.f16_apply_tiles(2112, 256 * nrb, ncu)['tail_rb'] >= 1:
            return 256 * nrb - 52
    raise AssertionError('no row count with a tail row block')


# id -> (S, M, N, options, abc, y outliers)
SHAPES = {
    'k132_n1': (2, 64, 1, {}, (-1.0, 0.0, -1.0), 0),
    'k132_n255': (2, 64, 255, {}, (-1.0, 0.0, -1.0), 0),
    'k132_n257': (2, 64, 257, {}, (-1.0, 0.0, -1.0), 0),
    'k640_n2300': (20, 300, 2300, {}, (-1.0, 0.0, -1.0), 0),
    'k640_n2300_fp32gram': (20, 300, 2300, {'f16_gram': 0}, (-1.0, 0.0, -1.0), 0),
    'k640_n71800_chunk640': (20, 300, 71800, {'gram_chunk': 640}, (-1.0, 0.0, -1.0), 0),
    'k2112_tail': (32, 1024, None, {}, (-1.0, 0.0, -1.0), 0),
    'k4224_n2000': (32, 2080, 2000, {}, (-1.0, 0.0, -1.0), 0),
    'k640_b+3': (20, 300, 2300, {}, (-1.0, 3.0, -1.0), 0),
    'k640_b-6': (20, 300, 2300, {}, (-1.0, -6.0, -1.0), 0),
    'k640_a-3': (20, 300, 2300, {}, (-3.0, 0.0, -1.0), 0),
    'k640_youtliers': (20, 300, 2300, {}, (-1.0, 0.0, -1.0), 5),
}


# the scale extremes: fp32 mode itself leaves the tier at b = +3 (cost 9.4e-6 against fp64 mode on the first GPU run, f16x3 7.9e-5:
# the fp16 Gram's accumulation amplified by cond(A)); there the gradient's 4x rule stands and the cost is reported only
SCALE_EXTREMES = ('k640_b+3', 'k640_b-6', 'k640_a-3', 'k640_youtliers')


def _data(S, M, N, abc, outliers, seed=0x5CF6F160):
    from scfgp_amd import synth
    seed += M + N
    X = synth.make_X(seed, N, D)
    y = synth.normal(seed + 1, 0, N).reshape(-1, 1)
    if outliers:                                    # a few rows with |y| >> typical: max |q| far above most rows' q
        y[np.arange(outliers) * (N // outliers)] = 1e3
    return X, y, synth.make_params(seed + 2, D, S, M, abc=abc)


def _engine(dtype, S, M, params, X, y, opts):
    from scfgp_amd.engine import HipEngine
    e = HipEngine(D, S, M, dtype)
    e.set_option('gram64', 0); e.set_option('apply_dma', 2); e.set_option('factor_form', 0)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_params(params); e.set_data(X, y)
    e.set_profiling(True)
    return e


def _reach(name, K, N, Np, Kp, opts, ncu):
    """the paths the shape is for, restated from the host code and asserted"""
    chunk = R.f16_chunk(Np, Kp, opts.get('gram_chunk', 4096))
    rows, nch, last = R.gram_chunks(Np, chunk)
    plan = R.f16_apply_tiles(K, Np, ncu)
    if name.startswith('k132'):
        assert K == 132 and Kp == 256 and not R.f16_apply_runs(K) and Np == 256 * (1 + (N > 256))
    if name.startswith('k640'):
        assert K == 640 and Kp == 640 and Kp // 128 == 5 and R.gram_tiles(Kp) == 11      # the A side's third 256-block sticks out
        assert plan['n256'] == 2 and [w for _, w in plan['main']] == [256, 256, 128]
    if name in ('k640_n2300', 'k640_n2300_fp32gram'):
        assert Np == 2304 and (rows, nch, last) == (1024, 3, 256)
    if name == 'k640_n71800_chunk640':
        assert Np == 71936 and rows == 1280 and rows % R.FOLD == 256 and (nch, last) == (57, 256)     # 2.5 folds per chunk
    if name == 'k2112_tail':
        assert Kp == 2176 and plan['n256'] == 8 and [w for _, w in plan['main']][-1] == 64 and plan['tail_rb'] >= 1
    if name == 'k4224_n2000':
        assert Kp == 4224 > 4096 and Kp // 128 == 33 and [w for _, w in plan['main']].count(128) == 1
    return plan, (rows, nch, last)


def _rule(e16, e32, floor=R.FLOOR_SPLIT):
    """block figures of the f16x3 context within 4x of the fp32 context's on the same block, plus the split's floor"""
    bad = {k: (v, e32[k]) for k, v in e16.items() if v > R.RULE * e32[k] + floor}
    return bad


class _Checks(list):
    """the walk's checks: every failure is collected (with its line) and reported at the end, so that one run shows them all"""
    def __call__(self, ok, msg=''):
        if not ok:
            line = 'line %d: %s' % (sys._getframe(1).f_lineno, msg)
            print('FAIL ' + line, flush=True)
            self.append(line)


class _Figs(list):
    """the per-stage figures, printed as they come (a failing assertion leaves the ones before it on the record)"""
    def __init__(self, name):
        super().__init__(); self.name = name

    def append(self, line):
        print('%s: %s' % (self.name, line), flush=True)
        super().append(line)


def _fig(blocks):
    w, k = R.worst(blocks)
    return '%.2e@%s' % (w, k)


def _walk(name, e, K, N, Kp, Np, y, f16):
    """step one context through the stages; returns what the checks need"""
    out = {}
    e.pass1()
    out['Phi'] = e.debug_read('Phi', (Np, Kp), np.float32)
    x1 = e.debug_read('G', (Kp * Kp + Kp + 8,))
    out['G'] = x1[:Kp * Kp].reshape(Kp, Kp); out['Gy'] = x1[Kp * Kp:Kp * Kp + Kp]
    if f16:
        out['Phi16'] = e.debug_read('Phi16', (Np, Kp), np.uint32)
        out['tmp1'] = e.debug_read('f16tmp', (8,), np.float32)
    assert e.factor()
    out['B'] = e.debug_read('B', (Kp, Kp)); out['vecs1'] = e.debug_read('vecs', (5, Kp))
    if f16:
        out['B16'] = e.debug_read('B16', (Kp, Kp), np.uint32); out['scaleB'] = e.debug_read('f16scale', (4,), np.float32)
    e.pass2(True)
    out['V'] = e.debug_read('V', (Np, Kp), np.float32)
    out['p'] = e.debug_read('p', (Np,)); out['q'] = e.debug_read('q', (Np,))
    x2 = e.debug_read('W', (Kp * Kp + Kp + 8,))
    out['W'] = x2[:Kp * Kp].reshape(Kp, Kp); out['Wp'] = x2[Kp * Kp:Kp * Kp + Kp]
    if f16:
        out['V16g'] = e.debug_read('V16g', (Np, Kp), np.uint32); out['qV16g'] = e.debug_read('qV16g', (Np, Kp), np.uint32)
        out['tmp2'] = e.debug_read('f16tmp', (8,), np.float32)
    e.adjoint()
    out['Abar'] = e.debug_read('Abar', (Kp, Kp)); out['vecs'] = e.debug_read('vecs', (5, Kp))
    if f16:
        out['A16'] = e.debug_read('B16', (Kp, Kp), np.uint32); out['scaleA'] = e.debug_read('f16scale', (4,), np.float32)
    e.pass3()
    out['Phibar'] = e.debug_read('V', (Np, Kp), np.float32)
    out['res'] = e.finish(True)
    out['names'] = [n for n, _ in e.timings()]
    return out


@pytest.mark.parametrize('name', list(SHAPES))
def test_f16x3_stage_walk(name):
    S, M, N, opts, abc, nout = SHAPES[name]
    ncu = _ncu()
    if N is None:
        N = _n_for_tail(ncu)
    X, y, params = _data(S, M, N, abc, nout)
    K = 2 * (S + M)
    ctx = {dt: _engine(dt, S, M, params, X, y, opts) for dt in ('f16x3', 'f32')}
    d = ctx['f16x3'].dims(); Kp, Np = d['Kp'], d['Np']
    plan, (rows, nch, last) = _reach(name, K, N, Np, Kp, opts, ncu)
    f16_gram = opts.get('f16_gram', 1) == 1
    runs = R.f16_apply_runs(K)
    a = _walk(name, ctx['f16x3'], K, N, Kp, Np, y, True)
    b = _walk(name, ctx['f32'], K, N, Kp, Np, y, False)
    yv = y.ravel()
    s = np.exp(params[1]) * np.sqrt(2.0 / M)
    figs = _Figs(name)
    chk = _Checks()
    tiles = (plan['main'] if runs else None)

    # ---- the f16 kernels ran (and the split of V only with the fp16 Gram)
    chk('split_phi' in a['names'] and ('split_v' in a['names']) == f16_gram, a['names'])
    chk('split_phi' not in b['names'])

    # ---- pass 1: Phi, its planes, the exponent
    chk(np.array_equal(a['Phi'].view(np.uint32), b['Phi'].view(np.uint32)))
    Phi32 = a['Phi']
    tmp1 = a['tmp1']
    chk(tmp1[0] == np.float32(s), (tmp1[0], s))
    eph = R.exponent(s)
    chk(tmp1[2] == np.float32(2.0 ** -eph) and (not f16_gram or tmp1[4] == np.float32(2.0 ** (-2 * eph))), tmp1)
    h, l, e_ = R.split_rows(Phi32, tmp1[0])
    chk(e_ == eph)
    Ph, Pl = R.decode_planes(a['Phi16'])
    chk(np.array_equal(R.encode_planes(h, l), a['Phi16']), 'Phi16 differs from the split of Phi in %d words' % np.sum(R.encode_planes(h, l) != a['Phi16']))
    chk(not a['Phi16'][N:].any() and not Ph[:, K:].any() and not Pl[:, K:].any())      # padding rows and columns are zero

    P64 = Phi32[:N, :K].astype(np.float64)
    absP = np.abs(P64)
    GT = absP.T @ absP
    offd = ~np.eye(K, dtype=bool)
    tblocks = lambda err: R.tile_errors(np.where(offd, err, 0.0), K)
    Gx = P64.T @ P64
    gy = P64.T @ yv; gy32 = P64.T @ yv.astype(np.float32).astype(np.float64); gyn = absP.T @ np.abs(yv)
    figs.append('Phi^T y vs fp64 sum f16x3 %.2e  f32 %.2e; vs fp32(y) f16x3 %.2e  f32 %.2e' % tuple(
        (np.abs(c['Gy'][:K] - g) / gyn).max() for g in (gy, gy32) for c in (a, b)))
    for c in (a, b):
        chk(not c['G'][K:].any() and not c['G'][:, K:].any())
    # the split pass sums Phi^T y in fp64 (fp32 mode's Gram, also the f16x3 context's with f16_gram = 0, carries y in fp32: 1.8e-8 of
    # sum |Phi| |y| on the first GPU run)
    if f16_gram:
        chk(np.all(np.abs(a['Gy'][:K] - gy) <= 1e-12 * gyn), 'Phi^T y is an fp64 sum')
    e16 = tblocks(R.normalised(a['G'][:K, :K], Gx, GT)); e32 = tblocks(R.normalised(b['G'][:K, :K], Gx, GT))
    figs.append('G vs exact     f16x3 %s  f32 %s' % (_fig(e16), _fig(e32)))
    chk(not _rule(e16, e32), _rule(e16, e32))
    if f16_gram:
        sc1 = float(tmp1[4])
        G3 = R.mirror_lower_tiles(R.gram3(Ph[:N, :K], Pl[:N, :K], Ph[:N, :K], Pl[:N, :K], sc1))
        e3 = R.tile_errors(R.normalised(a['G'][:K, :K], G3, GT), K)
        figs.append('G vs G3        f16x3 %s' % _fig(e3))
        chk(R.worst(e3)[0] <= R.CAP_GRAM3, figs[-1])
        off = {k: v for k, v in e3.items() if k[0] != k[1]}; dia = {k: v for k, v in e3.items() if k[0] == k[1]}
        chk(not R.outliers(off, R.CAP_GRAM3) and not R.outliers(dia, R.CAP_GRAM3), (R.outliers(off, R.CAP_GRAM3), R.outliers(dia, R.CAP_GRAM3)))
        # the diagonal: short of the exact sum of squares by the dropped l.l term, computable from the planes
        ll = (Pl[:N, :K].astype(np.float64) ** 2).sum(0) * sc1
        dg = np.diag(a['G'])[:K]; dx = np.diag(Gx)
        de = np.abs(dg - np.diag(G3)) / np.diag(GT)
        figs.append('G diagonal vs G3 %.2e, l.l shortfall %.2e of the diagonal' % (de.max(), (ll / np.diag(GT)).max()))
        chk(de.max() <= R.CAP_GRAM3)
        rep = (Ph[:N, :K].astype(np.float64) + Pl[:N, :K]) * 2.0 ** -eph
        chk(np.allclose(np.diag(G3) + ll, (rep ** 2).sum(0), rtol=1e-11, atol=0))

    # ---- factor: the operand's planes, the bound of |V|
    B = a['B']
    hB, lB, s0, s1 = R.split_operand(B, K, s)
    chk(np.array_equal(R.encode_planes(hB, lB), a['B16']), 'B16 differs from the split of B')
    chk(a['scaleB'][0] == np.float32(s0) and a['scaleB'][1] == np.float32(s1))
    tmp2 = a['tmp2']
    vb = R.v_bound(B, K, s, M)
    chk(abs(float(tmp2[5]) - vb) <= 2 * np.spacing(np.float32(vb)), (tmp2[5], vb))

    # ---- pass 2: V = Phi B, its planes, p and q, the weighted Gram
    V32 = a['V']
    chk(float(tmp2[5]) >= np.abs(V32[:N, :K]).max())
    if f16_gram:
        hv, lv, ev = R.split_rows(V32, tmp2[5])
        nd = np.sum(R.encode_planes(hv, lv) != a['V16g'])
        chk(nd == 0, 'V16g differs from the split of V in %d words (the epilogue claims bit-identity)' % nd)
        qv = a['q']
        chk(tmp2[6] == np.float32(np.abs(qv[:N]).max() * (1 + 1e-6)), (tmp2[6], np.abs(qv[:N]).max()))
        hq, lq, eq = R.split_rows_weighted(V32, qv, tmp2[5], tmp2[6])
        nq = np.sum(R.encode_planes(hq, lq) != a['qV16g'])
        chk(nq == 0, 'qV16g differs from its emulation in %d words' % nq)
        chk(tmp2[4] == np.float32(2.0 ** -(ev + eq)) and tmp2[2] == np.float32(2.0 ** -ev))
        chk(not a['V16g'][N:].any() and not a['qV16g'][N:].any())
    for c in (a, b):
        chk(not c['V'][N:].any() and not c['V'][:, K:].any())
    absPB = lambda Bm: absP @ np.abs(Bm[:K, :K])
    ablocks = lambda err: R.apply_errors(err, N, K, tiles)
    Vx16 = P64 @ B[:K, :K]; Vx32 = P64 @ b['B'][:K, :K]
    e16 = ablocks(R.normalised(V32[:N, :K], Vx16, absPB(B))); e32 = ablocks(R.normalised(b['V'][:N, :K], Vx32, absPB(b['B'])))
    figs.append('V vs exact     f16x3 %s  f32 %s' % (_fig(e16), _fig(e32)))
    chk(not _rule(e16, e32), _rule(e16, e32))
    if runs:
        V3 = R.apply3(Ph[:N], Pl[:N], hB, lB, float(a['scaleB'][0]))[:, :K]
        e3 = ablocks(R.normalised(V32[:N, :K], V3, absPB(B)))
        figs.append('V vs V3        f16x3 %s' % _fig(e3))
        chk(R.worst(e3)[0] <= R.CAP_APPLY3 and not R.outliers(e3, R.CAP_APPLY3), (figs[-1], R.outliers(e3, R.CAP_APPLY3)))
    # p and q from the fp64 formulas (oracle pass 2) on the device's Phi, B, alpha
    kappa = np.log1p(np.exp(params[2]))
    pq = {}
    for c in (a, b):
        al = c['vecs1'][1, :K]
        mu = P64 @ al; v = ((P64 @ c['B'][:K, :K]) * P64).sum(1); dd = kappa * (v + 1); r = mu - yv
        ee = 1 / dd - (r * r + v) / dd ** 2
        qx = 1 / dd + kappa * ee; px = 2 * r / dd
        rb = lambda u, x: {i: float(np.linalg.norm(u[i * 256:(i + 1) * 256] - x[i * 256:(i + 1) * 256]) /
                                    max(np.linalg.norm(x[i * 256:(i + 1) * 256]), 1e-300)) for i in range(-(-N // 256))}
        pq[id(c)] = (rb(c['p'][:N], px), rb(c['q'][:N], qx))
        chk(not c['p'][N:].any() and not c['q'][N:].any())
    for i, nm in ((0, 'p'), (1, 'q')):
        e16, e32 = pq[id(a)][i], pq[id(b)][i]
        figs.append('%s per row block f16x3 %s  f32 %s' % (nm, _fig(e16), _fig(e32)))
        chk(not _rule(e16, e32, 1e-6), _rule(e16, e32, 1e-6))
    # the weighted Gram and V^T p
    figs.append('V^T p vs fp64 sum f16x3 %.2e  f32 %.2e' % tuple(
        (np.abs(c['Wp'][:K] - c['V'][:N, :K].astype(np.float64).T @ c['p'][:N]) /
         (np.abs(c['V'][:N, :K].astype(np.float64)).T @ np.abs(c['p'][:N]))).max() for c in (a, b)))
    Va = a['V'][:N, :K].astype(np.float64)
    if f16_gram:                                                # from split_v's fp64 block partials
        chk(np.all(np.abs(a['Wp'][:K] - Va.T @ a['p'][:N]) <= 1e-12 * (np.abs(Va).T @ np.abs(a['p'][:N]))), 'V^T p is an fp64 sum')
    ex = {}
    for c in (a, b):
        Vc = c['V'][:N, :K].astype(np.float64); qc = c['q'][:N]
        ex[id(c)] = (Vc.T @ (qc[:, None] * Vc), np.abs(Vc).T @ (np.abs(qc)[:, None] * np.abs(Vc)))
    e16 = tblocks(R.normalised(a['W'][:K, :K], *ex[id(a)])); e32 = tblocks(R.normalised(b['W'][:K, :K], *ex[id(b)]))
    figs.append('W vs exact     f16x3 %s  f32 %s' % (_fig(e16), _fig(e32)))
    chk(not _rule(e16, e32), _rule(e16, e32))
    if f16_gram:
        Vh, Vl = R.decode_planes(a['V16g']); Qh, Ql = R.decode_planes(a['qV16g'])
        W3 = R.mirror_lower_tiles(R.gram3(Vh[:N, :K], Vl[:N, :K], Qh[:N, :K], Ql[:N, :K], float(tmp2[4])))
        e3 = R.tile_errors(R.normalised(a['W'][:K, :K], W3, ex[id(a)][1]), K)
        figs.append('W vs W3        f16x3 %s' % _fig(e3))
        chk(R.worst(e3)[0] <= R.CAP_GRAM3, figs[-1])
        off = {k: v for k, v in e3.items() if k[0] != k[1]}
        chk(not R.outliers(off, R.CAP_GRAM3), R.outliers(off, R.CAP_GRAM3))

    # ---- adjoint: Abar's planes
    hA, lA, sA, _ = R.split_operand(a['Abar'], K, s)
    chk(np.array_equal(R.encode_planes(hA, lA), a['A16']), 'B16 after the adjoint differs from the split of Abar')
    chk(a['scaleA'][0] == np.float32(sA))

    # ---- pass 3: Phibar = p alpha^T + y ut^T + 2 q o V + 2 Phi Abar
    eb = {}
    for c in (a, b):
        al = c['vecs'][1, :K]; ut = c['vecs'][3, :K]; pc = c['p'][:N]; qc = c['q'][:N]
        Vc = c['V'][:N, :K].astype(np.float64); Ab = c['Abar'][:K, :K]
        rest = np.outer(pc, al) + np.outer(yv, ut) + 2 * qc[:, None] * Vc
        x = rest + 2 * P64 @ Ab
        nrm = np.abs(np.outer(pc, al)) + np.abs(np.outer(yv, ut)) + 2 * np.abs(qc[:, None] * Vc) + 2 * absP @ np.abs(Ab)
        eb[id(c)] = ablocks(R.normalised(c['Phibar'][:N, :K], x, nrm)), rest, nrm
    e16, e32 = eb[id(a)][0], eb[id(b)][0]
    figs.append('Phibar vs exact f16x3 %s  f32 %s' % (_fig(e16), _fig(e32)))
    chk(not _rule(e16, e32), _rule(e16, e32))
    if runs:
        P3 = 2 * R.apply3(Ph[:N], Pl[:N], hA, lA, float(a['scaleA'][0]))[:, :K]
        e3 = ablocks(R.normalised(a['Phibar'][:N, :K] - eb[id(a)][1], P3, eb[id(a)][2]))
        figs.append('2 Phi Abar vs 3-term f16x3 %s' % _fig(e3))
        chk(R.worst(e3)[0] <= R.CAP_APPLY3 and not R.outliers(e3, R.CAP_APPLY3), (figs[-1], R.outliers(e3, R.CAP_APPLY3)))

    # ---- end to end: fp32 mode's tier against fp64 mode, and a bit-equal repeat
    from scfgp_amd.engine import HipEngine
    e64 = HipEngine(D, S, M, 'f64'); e64.set_params(params); e64.set_data(X, y)
    r64 = e64.eval(); e64.close()
    err = {}
    for nm, c in (('f16x3', a), ('f32', b)):
        cost, grad, alpha, Li = c['res']
        err[nm] = (abs(float(cost) - float(r64[0])) / max(1.0, abs(float(r64[0]))),
                   np.linalg.norm(grad - r64[1]) / np.linalg.norm(r64[1]))
    figs.append('cost / grad    f16x3 %.2e / %.2e  f32 %.2e / %.2e' % (err['f16x3'] + err['f32']))
    if err['f32'][0] < 1e-5 and err['f32'][1] < 1e-3 and name not in SCALE_EXTREMES:
        chk(err['f16x3'][0] < 1e-5 and err['f16x3'][1] < 1e-3, err)          # fp32 mode's parity tier
    chk(err['f16x3'][1] <= 4 * err['f32'][1] + 1e-6, err)
    again = _walk(name, ctx['f16x3'], K, N, Kp, Np, y, True)['res']
    chk(float(again[0]) == float(a['res'][0]) and np.array_equal(again[1], a['res'][1]))
    print('\n%s (K %d, N %d, Kp %d, Np %d, Gram chunk %d x %d, last %d, tail_rb %d):\n  %s' % (
        name, K, N, Kp, Np, rows, nch, last, plan['tail_rb'], '\n  '.join(figs)))
    for e in ctx.values():
        e.close()
    assert not chk, chk


def test_f16x3_state_between_calls():
    """full rows, a subset, the full rows again: the second full evaluation is bit-equal to the first (stale bounds, scales or planes
    -- f16tmp[6]'s max |q| is an atomicMax over a memset -- would show), and the subset's equals a fresh context's on X[idx]"""
    S, M, N = 20, 300, 2300
    X, y, params = _data(S, M, N, (-1.0, 0.0, -1.0), 0)
    e = _engine('f16x3', S, M, params, X, y, {})
    r1 = e.eval()
    idx = np.arange(0, N, 3)
    rs = e.eval_rows(idx)
    r2 = e.eval()
    assert float(r1[0]) == float(r2[0]) and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])
    names = [n for n, _ in e.timings()]
    assert 'split_phi' in names and 'split_v' in names
    e.close()
    f = _engine('f16x3', S, M, params, np.ascontiguousarray(X[idx]), np.ascontiguousarray(y[idx]), {})
    rf = f.eval()
    f.close()
    assert float(rs[0]) == float(rf[0]) and np.array_equal(rs[1], rf[1]) and np.array_equal(rs[2], rf[2])


def test_f16x3_debug_names_refused_outside_the_mode():
    from scfgp_amd.engine import HipEngine
    for dt in ('f32', 'f64'):
        e = HipEngine(D, 2, 64, dt)
        for nm in ('Phi16', 'V16g', 'qV16g', 'B16', 'f16scale', 'f16tmp'):
            with pytest.raises(Exception):
                e.debug_read(nm, (8,), np.float32)
            assert nm in e.last_error() and 'F16X3' in e.last_error()
        e.close()
