"""Time scfgp_forget at the headline shape (D=64, S=32, M=1024), per dtype and number of removed rows, in its three forms -- factors
only, predictions only (Li' never leaves the device), both -- next to scfgp_condition on the same rows and next to what removing rows
costs without it: one forward-only evaluation (want_grad=0) from host arrays on the remaining rows.  The fit is a forward evaluation
over N0 synthetic rows; the removed rows are its first n.  Prints one JSON line with wall times from host arrays to host arrays (best
of two calls; the first call of each kind, which allocates, is not timed), and whether the predictions-only form was not slower than
the form that also downloads Li'.
Usage: python tools/forget_time.py [--once] [--no-eval] [--n0 ROWS] [n ...]      (default: 1 4096 32768 262144; N0 = 1e6)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd import synth
from scfgp_amd.engine import HipEngine

argv = sys.argv[1:]
once = '--once' in argv
no_eval = '--no-eval' in argv
N0 = int(argv[argv.index('--n0') + 1]) if '--n0' in argv else 1000000
skip = {argv.index('--n0') + 1} if '--n0' in argv else set()
ns = [int(a) for i, a in enumerate(argv) if not a.startswith('-') and i not in skip] or [1, 4096, 32768, 262144]
D, S, M = 64, 32, 1024
K = 2 * (S + M)
params = synth.make_params(11, D, S, M, abc=(-1.0, 0.0, -1.0))
rng = np.random.default_rng(7)
assert max(ns) < N0, 'the removed rows are rows of the fit, and some must remain'


def best(f, reps=2):
    ts = []
    for _ in range(1 if once else reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


X0 = synth.make_X(5, N0, D)
y0 = np.sin(3.0 * X0[:, :1]) + 0.1 * rng.standard_normal((N0, 1))
out = {}
for dt in ('f64', 'f32'):
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    eng.set_data(X0, y0)
    _, _, alpha, Li = eng.eval(want_grad=False)
    alpha, Li = alpha.copy(), Li.copy()
    eng.condition(X0[:256], y0[:256], alpha, Li)
    eng.forget(X0[:256], y0[:256], alpha, Li, factors=True, predict=True)    # first calls: allocations
    for n in ns:
        Xo, yo = X0[:n], y0[:n]
        if n > 32768:
            eng.forget(Xo, yo, alpha, Li)                                    # the slabs of a full chunk
        r = {'forget_factors_s': best(lambda: eng.forget(Xo, yo, alpha, Li)),
             'forget_predict_s': best(lambda: eng.forget(Xo, yo, alpha, Li, factors=False, predict=True)),
             'forget_both_s': best(lambda: eng.forget(Xo, yo, alpha, Li, factors=True, predict=True)),
             'condition_s': best(lambda: eng.condition(Xo, yo, alpha, Li))}
        r['min_pivot2'] = eng.forget(Xo, yo, alpha, Li, factors=False, predict=True)[2]['min_pivot2']
        r['predict_only_not_slower_than_both'] = bool(r['forget_predict_s'] <= r['forget_both_s'])
        out['%s_n%d' % (dt, n)] = r
    if not no_eval:                                                          # last: these calls replace the resident rows
        for n in ns:
            Xr, yr = np.ascontiguousarray(X0[n:]), np.ascontiguousarray(y0[n:])
            eng.eval(Xr, yr, want_grad=False)
            out['%s_n%d' % (dt, n)]['eval_forward_remaining_s'] = best(lambda: eng.eval(Xr, yr, want_grad=False))
    eng.close()
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'N0': N0, 'forget': out}))
