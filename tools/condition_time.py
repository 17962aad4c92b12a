"""Time scfgp_condition next to scfgp_predict on the same rows at the headline shape (D=64, S=32, M=1024), per dtype and number of new
rows, and next to what absorbing rows costs without it: one forward-only evaluation (want_grad=0) over a resident set of N0 synthetic
rows.  Prints one JSON line with wall times from host arrays to host arrays (best of two calls; the first call of each kind, which
allocates, is not timed).  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/condition_time.py --once --no-eval 4096
Usage: python tools/condition_time.py [--once] [--no-eval] [--n0 ROWS] [n ...]      (default: 1 256 4096 32768 262144; N0 = 1e6)"""
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
ns = [int(a) for i, a in enumerate(argv) if not a.startswith('-') and i not in skip] or [1, 256, 4096, 32768, 262144]
D, S, M = 64, 32, 1024
K = 2 * (S + M)
params = synth.make_params(11, D, S, M, abc=(-1.0, 0.0, -1.0))
rng = np.random.default_rng(7)


def best(f, reps=2):
    ts = []
    for _ in range(1 if once else reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


Xn = synth.make_X(3, max(ns), D)
yn = np.sin(3.0 * Xn[:, 0]) + 0.1 * rng.standard_normal(max(ns))
if not no_eval:
    X0 = synth.make_X(5, N0, D)
    y0 = np.sin(3.0 * X0[:, :1]) + 0.1 * rng.standard_normal((N0, 1))
out = {}
for dt in ('f64', 'f32'):
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    if no_eval:                                                     # a synthetic posterior: any lower-triangular factor times the update
        alpha = rng.standard_normal(K) / np.sqrt(K)
        Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K)
    else:
        eng.set_data(X0, y0)
        _, _, alpha, Li = eng.eval(want_grad=False)
        alpha, Li = alpha.copy(), Li.copy()
        out['%s_eval_forward_N0_s' % dt] = best(lambda: eng.eval(want_grad=False))
    eng.predict(Xn[:256], alpha, Li)
    eng.condition(Xn[:256], yn[:256], alpha, Li)                    # first calls: allocations
    for n in ns:
        if n > 32768:
            eng.condition(Xn[:n], yn[:n], alpha, Li)                # the slabs of a full chunk
        out['%s_n%d' % (dt, n)] = {'condition_s': best(lambda: eng.condition(Xn[:n], yn[:n], alpha, Li)),
                                    'predict_s': best(lambda: eng.predict(Xn[:n], alpha, Li))}
    eng.close()
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'N0': None if no_eval else N0, 'condition': out}))
