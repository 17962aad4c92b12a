"""Time scfgp_predict and scfgp_predict_grad (mean only, and with the std gradient) at the headline shape (D=64, S=32, M=1024), per
dtype and test-set size; prints one JSON line with rows/s.
Usage: python tools/predict_grad_time.py [T ...]      (default: 262144 1000000)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.engine import HipEngine, num_params

Ts = [int(a) for a in sys.argv[1:]] or [262144, 1000000]
D, S, M = 64, 32, 1024
K = 2 * (S + M)
rng = np.random.default_rng(7)
params = 0.1 * rng.standard_normal(num_params(D, S, M))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


out = {}
for T in Ts:
    Xs = rng.standard_normal((T, D))
    for dt in ('f64', 'f32'):
        eng = HipEngine(D, S, M, dtype=dt)
        eng.set_params(params)
        eng.predict_grad(Xs[:4096], alpha, Li)                 # first call: allocations
        tp = best(lambda: eng.predict(Xs, alpha, Li))
        tm = best(lambda: eng.predict_grad(Xs, alpha, Li, want_std=False))
        ts = best(lambda: eng.predict_grad(Xs, alpha, Li))
        out['%s_T%d' % (dt, T)] = {'predict_s': tp, 'grad_mean_s': tm, 'grad_std_s': ts, 'predict_rows_per_s': T / tp,
                                   'grad_mean_rows_per_s': T / tm, 'grad_std_rows_per_s': T / ts}
        eng.close()
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'predict_grad': out}))
