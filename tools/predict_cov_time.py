"""Time scfgp_predict_cov (symmetric form) next to scfgp_predict at the headline shape (D=64, S=32, M=1024), per dtype and test-set
size; prints one JSON line with wall times from host arrays to the host array.  The wall time includes the copy of the T x T fp64
result to pageable host memory (2 GB at T = 16384); `host_copy_s` times a plain host-side copy of an array of that size for scale.
Kernel times come from a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/predict_cov_time.py --once 16384
Usage: python tools/predict_cov_time.py [--once] [T ...]      (default: 1024 4096 16384; --once: one timed call per dtype and T)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.engine import HipEngine, num_params

once = '--once' in sys.argv[1:]
Ts = [int(a) for a in sys.argv[1:] if not a.startswith('-')] or [1024, 4096, 16384]
D, S, M = 64, 32, 1024
K = 2 * (S + M)
rng = np.random.default_rng(7)
params = 0.1 * rng.standard_normal(num_params(D, S, M))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)


def best(f, reps=2):
    ts = []
    for _ in range(1 if once else reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


out = {}
for T in Ts:
    Xs = rng.standard_normal((T, D))
    for dt in ('f64', 'f32'):
        eng = HipEngine(D, S, M, dtype=dt)
        eng.set_params(params)
        eng.predict(Xs[:256], alpha, Li)
        eng.predict_cov(Xs[:256], Li)                               # first calls: allocations
        rec = {'predict_s': best(lambda: eng.predict(Xs, alpha, Li))}
        rec['predict_cov_s'] = best(lambda: eng.predict_cov(Xs, Li))
        rec['predict_cov_noise_s'] = best(lambda: eng.predict_cov(Xs, Li, noise=True), reps=1)
        rec['predict_cov_cross_256_s'] = best(lambda: eng.predict_cov(Xs, Li, Xb=Xs[:256]))
        src = np.empty((T, T))
        src.fill(1.0)
        rec['host_copy_s'] = best(lambda: np.copyto(np.empty_like(src), src), reps=1)
        rec['flops'] = 2.0 * T * T * K
        out['%s_T%d' % (dt, T)] = rec
        eng.close()
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'predict_cov': out}))
