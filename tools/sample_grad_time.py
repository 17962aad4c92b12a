"""Time scfgp_sample_grad against scfgp_predict_grad (mean gradient only) at the same T on the same build, at the headline shape
(D=64, S=32, M=1024), per dtype, row count and sample count, with random sidx; and one continuous maximisation of 64 sample functions
(the steps of SCFGP.sample_maximize on the engine: sample_argmax over a pool, sample_weights, ascent by sample_grad).  Prints one JSON
line.  T = 262144 is the "many rows share few samples" case (the weight reads are L2 hits); T = 1024 with nsamp = 1024 is the "one row
per sample" case (every weight row is read once: latency-bound).
Usage: python tools/sample_grad_time.py [T ...]      (default: 262144 1024)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.ascent import ascend
from scfgp_amd.engine import HipEngine, num_params

Ts = [int(a) for a in sys.argv[1:]] or [262144, 1024]
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
for dt in ('f64', 'f32'):
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    eng.predict_grad(rng.standard_normal((4096, D)), alpha, Li, want_std=False)      # first call: allocations
    Ws = {ns: eng.sample_weights(alpha, Li, ns, seed=1) for ns in (64, 1024)}
    for T in Ts:
        Xs = rng.standard_normal((T, D))
        rec = {'predict_grad_mean_s': best(lambda: eng.predict_grad(Xs, alpha, Li, want_std=False))}
        for ns, W in Ws.items():
            sidx = rng.integers(0, ns, T)
            t = best(lambda: eng.sample_grad(Xs, W, sidx=sidx))
            rec['sample_grad_nsamp%d_s' % ns] = t
            rec['sample_grad_nsamp%d_rows_per_s' % ns] = T / t
        rec['predict_grad_mean_rows_per_s'] = T / rec['predict_grad_mean_s']
        out['%s_T%d' % (dt, T)] = rec
    # one maximisation: 64 sample functions from their best rows of a 4096-row pool, in the box the pool spans
    ns, pool = 64, rng.standard_normal((4096, D))
    t0 = time.perf_counter()
    idx, _ = eng.sample_argmax(pool, alpha, Li, ns, seed=1)
    W = eng.sample_weights(alpha, Li, ns, seed=1)
    Xb, val, conv, n_calls = ascend(lambda X, s: eng.sample_grad(X, W, sidx=s), pool[idx], np.arange(ns), pool.min(0), pool.max(0))
    out['%s_maximize' % dt] = {'nsamp': ns, 'pool': 4096, 'seconds': time.perf_counter() - t0, 'sample_grad_calls': n_calls,
                               'converged': int(conv.sum())}
    eng.close()
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'sample_grad': out}))
