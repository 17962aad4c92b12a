"""Bit identity of the posterior entry points and of the evaluation between two builds of the library (default: '_head', the parent
commit's build made by tools/build_head.sh, and '', the working tree's).  For each variant in turn a fresh child process -- one on the GPU at a time, under a
time limit of its own; this process never opens the GPU -- runs a fixed, seeded list of calls and writes a SHA-256 per output array.
Then a table, and exit status 1 on any difference.  A child that fails or runs out of time ends the run.

The list, for f32 and f64, at (D, S, M) = (5, 4, 60) with 65 836 rows (three chunks of 32 768: the buffers of the chunk pipeline are
reused) and at (20, 20, 280) with 5000 rows: predict, predict_raw, predict_y with targets (metrics included); predict_grad in its three
modes with and without the std gradient; sample_weights; sample in its three modes with and without noise, 3 samples; predict_cov
symmetric at 2500 rows, cross at all rows x 50 and at 2500 x 9000 (two panels per chunk); condition in both modes; loo with blocks
1, 7, 64 from host rows and block 7 on resident rows; select without weights and with weights around the chunk boundaries, with
std_after; predict_gradcov with all four outputs and weights over three chunks, in raw mode, and with its default outputs over all rows;
predict_pd with all four outputs and weights over all rows for three dimensions, in raw mode, and with its default outputs for every
dimension; condition_grad over three chunks of whole points with values and a rho that holds zeros, and in raw mode along two dims; sobol
with all five outputs for 40 sampled columns under a mixed measure (each of the last four where the build has it: outputs that only one
build produces are listed as new, not as different); with
weights that are zero across every chunk boundary, at both shapes, sample_argmax in mode y with and without them, acquire in raw mode for
its five kinds (ei with grad), acquire_kg symmetric and with Xr with the node table, select_iv with Xr and wr and as its own reference;
at the second shape sample_grad with sidx, select_qei with pending rows and forget (a refusal is compared as its text).  Then the
evaluation side, at both shapes: eval with gradient on the rows (cost, grad, alpha, Li) and three adam iterations of train (cost
history, alpha, Li).  With three
variants (_head,_head,) the first two runs tell which outputs are not bit-stable from run to run: those are marked, not compared.  The factors are a synthetic posterior (tools/select_time.py's): identity of the bits does not depend on their values.
Usage: python tools/posterior_ab.py [--variants _head,] [--limit SECONDS]        (default limit: 300 per child)
       python tools/posterior_ab.py --child OUT.json                             (the list, in this process, on SCFGP_LIB_VARIANT)"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(5, 4, 60, 65536 + 300), (20, 20, 280, 5000)]


def digest(a):
    if isinstance(a, dict):
        a = np.array([a[k] for k in sorted(a)], np.float64)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def calls(D, S, M, n, dt):
    """yields (name, tuple of output arrays)"""
    from scfgp_amd import synth
    from scfgp_amd.engine import HipEngine
    from scfgp_amd.scaler import Scaler
    K = 2 * (S + M)
    rng = np.random.default_rng(7)
    params = synth.make_params(11, D, S, M, abc=(-1.0, 0.0, -1.0))
    X = synth.make_X(3, n, D)
    y = np.sin(3 * X[:, :1]) + 0.1 * rng.standard_normal((n, 1))
    Li = 0.02 * (np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K))
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Xr = 1.5 * X + 0.25                                         # "raw" rows whose scaler maps them back near X
    xs = Scaler('normal'); xs.fit(Xr)
    ys = Scaler('min-max'); ys.fit(y)
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    eng.set_x_scaler(xs); eng.set_y_scaler(ys)
    yield 'predict', eng.predict(X, alpha, Li)
    yield 'predict_raw', eng.predict_raw(Xr, alpha, Li)
    yield 'predict_y', eng.predict_y(Xr, alpha, Li, ys=y)
    for mode in ('scaled', 'raw', 'y'):
        for want_std in (False, True):
            out = eng.predict_grad(Xr if mode != 'scaled' else X, alpha, Li, mode=mode, want_std=want_std)
            yield 'predict_grad %s std=%d' % (mode, want_std), out[:3] + ((out[3],) if want_std else ())
    yield 'sample_weights', (eng.sample_weights(alpha, Li, 3, seed=5),)
    for mode in ('scaled', 'raw', 'y'):
        for noise in (False, True):
            yield 'sample %s noise=%d' % (mode, noise), (eng.sample(Xr if mode != 'scaled' else X, alpha, Li, 3, seed=5, mode=mode, noise=noise),)
    yield 'predict_cov sym 2500', (eng.predict_cov(X[:2500], Li, noise=True),)
    yield 'predict_cov cross %d x 50' % n, (eng.predict_cov(X, Li, Xb=X[100:150]),)
    Xb = synth.make_X(4, 9000, D)
    yield 'predict_cov cross 2500 x 9000 raw', (eng.predict_cov(Xr[:2500], Li, Xb=1.5 * Xb + 0.25, mode='raw'),)
    yield 'condition scaled', eng.condition(X, y, alpha, Li)
    yield 'condition raw', eng.condition(Xr, y, alpha, Li, mode='raw')
    for block in (1, 7, 64):
        out = eng.loo(X, y, alpha, Li, block=block)
        yield 'loo block %d' % block, out[:3] + (out[3],)
    eng.set_data(X, y)
    out = eng.loo(None, None, alpha, Li, block=7)
    yield 'loo resident block 7', out[:3] + (out[3],)
    yield 'select', eng.select(X, Li, 8, return_std=True)
    w = np.zeros(n)
    for b in range(32768, n, 32768):
        w[b - 25:b + 25] = 1.0
    if not w.any():
        w[n // 2 - 25:n // 2 + 25] = 1.0
    yield 'select weights raw', eng.select(Xr, Li, 8, w=w, raw=True, return_std=True)
    if hasattr(eng.lib, 'scfgp_predict_gradcov'):                # a build of an older commit lacks it: its outputs are listed as new
        allout = ('dmu', 'dvar', 'dcov', 'asub')
        n3 = min(n, 2 * eng.gradcov_points_per_chunk(True) + 3)   # three chunks where the call has the rows for them
        out = eng.predict_gradcov(X[:n3], alpha, Li, w=w[:n3] + 0.5, want=allout)
        yield 'predict_gradcov scaled %d rows' % n3, tuple(out[k] for k in allout)
        out = eng.predict_gradcov(Xr[:2500], alpha, Li, mode='raw', want=allout)
        yield 'predict_gradcov raw 2500 rows', tuple(out[k] for k in allout)
        out = eng.predict_gradcov(X, alpha, Li)
        yield 'predict_gradcov scaled %d rows, default outputs' % n, tuple(out[k] for k in ('dmu', 'dvar', 'asub'))
    if hasattr(eng.lib, 'scfgp_predict_pd'):                     # the same: new in a build that has it
        allpd = ('pd', 'sd', 'cov', 'ice')
        dims = [0, D - 1, D // 2]
        lo, hi = X[:, dims].min(0), X[:, dims].max(0)
        grid = lo[:, None] + (hi - lo)[:, None] * np.linspace(0.0, 1.0, 7)[None, :]
        out = eng.predict_pd(X, alpha, Li, dims, grid, w=w + 0.5, want=allpd)
        yield 'predict_pd scaled %d rows' % n, tuple(out[k] for k in allpd)
        out = eng.predict_pd(Xr[:2500], alpha, Li, dims, 1.5 * grid + 0.25, mode='raw', want=allpd)
        yield 'predict_pd raw 2500 rows', tuple(out[k] for k in allpd)
        out = eng.predict_pd(X, alpha, Li, list(range(D)), np.tile(np.linspace(0.1, 0.9, 5), (D, 1)))
        yield 'predict_pd scaled %d rows, every dimension, default outputs' % n, tuple(out[k] for k in ('pd', 'sd'))
    if hasattr(eng.lib, 'scfgp_condition_grad'):                 # the same: new in a build that has it
        n3 = min(n, 2 * eng.condition_grad_points_per_chunk(D, True) + 3)      # three chunks of whole points
        Gd = rng.standard_normal((n3, D))
        rz = rng.choice([0.0, 0.25, 1.0, 100.0], size=(n3, D))
        yield 'condition_grad scaled %d points, values, rho with zeros' % n3, eng.condition_grad(X[:n3], Gd, alpha, Li, rho=rz, y=y[:n3])
        yield 'condition_grad raw 2500 points, dims', eng.condition_grad(Xr[:2500], Gd[:2500, [D - 1, 0]], alpha, Li, dims=[D - 1, 0], raw=True)
    if hasattr(eng.lib, 'scfgp_sobol'):                          # the same: new in a build that has it
        kind = (np.arange(D) % 2).astype(np.int32)
        out = eng.sobol(kind, np.where(kind == 1, 0.5, 0.0), np.where(kind == 1, 0.25, 1.0), eng.sample_weights(alpha, Li, 40, seed=5),
                        want=('f0', 'V', 'Vmain', 'Vtot', 'phibar'))
        yield 'sobol mixed measure, 40 sampled columns, all outputs', tuple(out[k] for k in ('f0', 'V', 'Vmain', 'Vtot', 'phibar'))
    # the pool entry points: those that feed weights as targets at both shapes (wz: zero across every chunk boundary), the rest at the
    # second shape only
    wz = np.ones(n)
    for b in range(32768, n, 32768):
        wz[b - 25:b + 25] = 0.0
    wz[n // 3:n // 3 + 40] = 0.0
    nr = min(n, 3000)

    def attempt(fn, keys=None):                                  # a refusal is compared as its text
        try:
            out = fn()
            return tuple(np.asarray(out[k]) for k in keys) if keys else out
        except (np.linalg.LinAlgError, FloatingPointError) as e:
            return (np.frombuffer(str(e).encode(), np.uint8),)
    for ww, tag in ((None, ''), (wz, ' weights')):
        yield 'sample_argmax y' + tag, attempt(lambda: eng.sample_argmax(Xr, alpha, Li, 3, seed=5, w=ww, mode='y'))
    for kind, kw in (('ucb', dict(beta=2.0)), ('pi', dict(best=0.3)), ('ei', dict(best=0.3, xi=0.01)), ('logei', dict(best=0.3)),
                     ('mes', dict(fstar=np.array([0.9, 1.1, 1.4])))):
        want = ('acq', 'argmax', 'mu', 'sd') + (('grad',) if kind == 'ei' else ())
        yield ('acquire %s raw weights' % kind,
               attempt(lambda: eng.acquire(Xr, alpha, Li, kind, w=wz, mode='raw', want=want, **kw), ('acq', 'idx', 'val', 'mu', 'sd') + want[4:]))
    kgw = ('kg', 'kg_hi', 'idx', 'val', 'm', 's')
    yield 'acquire_kg symmetric %d rows' % nr, attempt(lambda: eng.acquire_kg(X[:nr], alpha, Li, w=wz[:nr], want=kgw), kgw)
    yield 'acquire_kg %d x %d' % (n, nr), attempt(lambda: eng.acquire_kg(X, alpha, Li, Xr=X[100:100 + nr], w=wz, want=kgw), kgw)
    yield 'select_iv Xr wr', attempt(lambda: eng.select_iv(X, Li, 8, Xr=X[:nr] + 0.01, w=wz, wr=wz[:nr] + 0.5, return_std=True))
    yield 'select_iv own reference wr', attempt(lambda: eng.select_iv(X, Li, 8, wr=wz, return_std=True))
    if n <= 5000:
        W = eng.sample_weights(alpha, Li, 4, seed=5)
        yield 'sample_grad sidx y', attempt(lambda: eng.sample_grad(Xr, W, sidx=(np.arange(n) * 7) % 4, mode='y'))
        yield 'select_qei pending', attempt(lambda: eng.select_qei(X, alpha, Li, 8, 16, 0.3, xi=0.01, seed=5, w=wz, pending=X[:3] + 0.05,
                                                                   return_score0=True, return_state=True))
        for rows in (n, 64):                                    # most likely refused: these rows are not in the synthetic fit
            yield 'forget %d rows' % rows, attempt(lambda: eng.forget(X[:rows], y[:rows], alpha, Li, factors=True, predict=True))
    # the evaluation side, last, so that the calls above run on the context as they always did
    cost, grad, a1, L1 = eng.eval(X, y)
    yield 'eval with gradient', (cost, grad, a1.copy(), L1.copy())
    eng.opt_init('adam')
    yield 'train 3 iterations', eng.train(3)
    eng.close()


def child(out_path):
    res = {}
    for D, S, M, n in SHAPES:
        for dt in ('f32', 'f64'):
            for name, arrays in calls(D, S, M, n, dt):
                for k, a in enumerate(arrays):
                    res['%s (%d,%d,%d) n=%d | %s | %d' % (dt, D, S, M, n, name, k)] = digest(a)
    with open(out_path, 'w') as f:
        json.dump(res, f)
    return 0


def main(argv):
    if argv[:1] == ['--child']:
        return child(argv[1])
    variants = argv[argv.index('--variants') + 1].split(',') if '--variants' in argv else ['_head', '']
    limit = argv[argv.index('--limit') + 1] if '--limit' in argv else '300'
    got = []
    with tempfile.TemporaryDirectory() as tmp:
        for v in variants:
            out = os.path.join(tmp, 'hashes%s.json' % v)
            r = subprocess.run(['timeout', '-k', '10', limit, sys.executable, os.path.abspath(__file__), '--child', out], cwd=ROOT,
                               env=dict(os.environ, SCFGP_LIB_VARIANT=v))
            if r.returncode != 0:
                print('variant %r failed: exit status %d' % (v, r.returncode), flush=True)
                return r.returncode
            with open(out) as f:
                got.append(json.load(f))
    # three variants: the first two (the same build twice) tell which outputs are not bit-stable from run to run
    unstable = {k for k in set(got[0]) | set(got[1]) if got[0].get(k) != got[1].get(k)} if len(got) == 3 else set()
    a, b = got[-2:]
    variants = variants[-2:]
    bad = 0
    print('%-78s %-14s %-14s' % ('dtype shape | call | output', repr(variants[0]), repr(variants[1])))
    new = 0
    for key in sorted(set(a) | set(b)):
        only = key not in a or key not in b                     # an entry point that one of the builds lacks: nothing to compare
        same = a.get(key) == b.get(key)
        bad += not same and not only and key not in unstable
        new += only
        print('%-78s %-14s %-14s %s' % (key, a.get(key, '-')[:12], b.get(key, '-')[:12], 'unstable (differs between two runs of one build)'
                                        if key in unstable else 'new' if only else 'same' if same else 'DIFFERENT'))
    print('%d outputs, %d different, %d in one build only, %d unstable' % (len(set(a) | set(b)), bad, new, len(unstable)), flush=True)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]) or 0)
