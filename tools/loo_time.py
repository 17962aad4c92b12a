"""Time scfgp_loo next to scfgp_predict on the same rows at the headline shape (D=64, S=32, M=1024), per dtype, block size and number of
rows; the largest row count is also run on the resident rows (X = None: no upload).  Prints one JSON line per case with wall times
from host arrays to host arrays (best of two calls; the first call of each kind, which allocates, is not timed).  The factors are a
synthetic posterior scaled so that every I - H is positive definite: the cost does not depend on their values.  Kernel times come
from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/loo_time.py --once --dtype f32 --blocks 16 32768
Usage: python tools/loo_time.py [--once] [--dtype f32|f64] [--blocks B,B,..] [n ...]      (default: both, 1,16,64; 32768 262144 1000000)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd import synth
from scfgp_amd.engine import HipEngine

argv = sys.argv[1:]
once = '--once' in argv
skip = set()


def opt(name, default):
    if name in argv:
        skip.add(argv.index(name) + 1)
        return argv[argv.index(name) + 1]
    return default


dtypes = [d for d in opt('--dtype', 'f32,f64').split(',')]
blocks = [int(b) for b in opt('--blocks', '1,16,64').split(',')]
ns = [int(a) for i, a in enumerate(argv) if not a.startswith('-') and i not in skip] or [32768, 262144, 1000000]
D, S, M = 64, 32, 1024
K = 2 * (S + M)
params = synth.make_params(11, D, S, M, abc=(-1.0, 0.0, -1.0))
rng = np.random.default_rng(7)


def best(f, reps=2):
    ts = []
    for _ in range(1 if once else reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


X = synth.make_X(3, max(ns), D)
y = (np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(max(ns)))[:, None]
# |phi|^2 = 2 e^{2b} = 2: with |Li|_2 <= 0.05 every h is below 0.005 and a block of 64 rows keeps lambda_max(H) below 0.32
Li = 0.02 * (np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K))
alpha = rng.standard_normal(K) / np.sqrt(K)
for dt in dtypes:
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    eng.predict(X[:256], alpha, Li)
    eng.loo(X[:256], y[:256], alpha, Li, block=1)                    # first calls: allocations
    for n in ns:
        t_pred = best(lambda: eng.predict(X[:n], alpha, Li))
        resident = n == max(ns)
        if resident:
            eng.set_data(np.ascontiguousarray(X[:n]), np.ascontiguousarray(y[:n]))
        for b in blocks:
            rec = {'D': D, 'S': S, 'M': M, 'K': K, 'dtype': dt, 'n': n, 'block': b, 'predict_s': t_pred,
                   'loo_s': best(lambda: eng.loo(X[:n], y[:n], alpha, Li, block=b))}
            if resident:
                rec['loo_resident_s'] = best(lambda: eng.loo(None, None, alpha, Li, block=b))
            rec['loo_over_predict'] = rec['loo_s'] / t_pred
            print(json.dumps(rec), flush=True)
    eng.close()
