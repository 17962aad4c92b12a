"""Time scfgp_sample (Phi* W for nsamp posterior sample functions) next to scfgp_predict at the headline shape (D=64, S=32, M=1024), per
dtype, test-set size and sample count; prints one JSON line with wall times and rows/s.  The wall time includes the copy of the
T x nsamp fp64 output to pageable host memory (2 GB at T = 10^6, nsamp = 256); `host_copy_s` times a plain host-side copy of an array
of that size for scale.
Usage: python tools/sample_time.py [T ...]      (default: 262144 1000000)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.engine import HipEngine, num_params

Ts = [int(a) for a in sys.argv[1:]] or [262144, 1000000]
NS = [16, 64, 256]
D, S, M = 64, 32, 1024
K = 2 * (S + M)
rng = np.random.default_rng(7)
params = 0.1 * rng.standard_normal(num_params(D, S, M))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)


def best(f, reps=2):
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
        eng.predict(Xs[:4096], alpha, Li)
        eng.sample(Xs[:4096], alpha, Li, 16)                      # first calls: allocations
        tp = best(lambda: eng.predict(Xs, alpha, Li))
        rec = {'predict_s': tp, 'predict_rows_per_s': T / tp}
        tw = best(lambda: eng.sample_weights(alpha, Li, 256))
        rec['weights_256_s'] = tw
        for ns in NS:
            ts = best(lambda: eng.sample(Xs, alpha, Li, ns))
            tn = best(lambda: eng.sample(Xs, alpha, Li, ns, noise=True), reps=1)
            src = np.empty((T, ns))
            src.fill(1.0)
            th = best(lambda: np.copyto(np.empty_like(src), src), reps=1)
            rec['ns%d' % ns] = {'sample_s': ts, 'sample_noise_s': tn, 'rows_per_s': T / ts, 'host_copy_s': th}
        out['%s_T%d' % (dt, T)] = rec
        eng.close()
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'sample': out}))
