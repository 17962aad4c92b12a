"""Time scfgp_condition_grad in fp32 contexts (and, beside them, fp64 ones) at the headline shape H (D=64, S=32, M=1024) and at C2's
(D=32, S=16, M=256): the host wall time of one call that absorbs n points with all D derivatives and their values (nb = D + 1 rows a
point, n such that the call has three chunks), next to scfgp_condition on n (D + 1) rows -- the same C and Gram row count and D + 1
times the feature-map work; in an fp32 context in fp32 products, where condition_grad's first pass is fp64, in an fp64 context in the
same products -- and the event times of the call's own kernels, summed over its chunks, against bytes / HBM rate (the row kernel reads
np Kp doubles and writes np nb Kp).  Best of three after a warm-up.  Writes profiles/condgrad_time_line.json and prints it.
Usage: python tools/condition_grad_time.py [OUT.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.engine import HipEngine, num_params

HBM_GBS = 8000.0
SHAPES = {'H': (64, 32, 1024), 'C2': (32, 16, 256)}
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'condgrad_time_line.json')


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


res = {}
rng = np.random.default_rng(7)
for cfg, dt in [(c, d) for c in SHAPES for d in ('f32', 'f64')]:
    D, S, M = SHAPES[cfg]
    K = 2 * (S + M)
    Kp = -(-K // 128) * 128
    nb = D + 1
    eng = HipEngine(D, S, M, dtype=dt)
    npts = eng.condition_grad_points_per_chunk(D, True)
    n = 2 * npts + 3                                               # three chunks
    params = 0.1 * rng.standard_normal(num_params(D, S, M))
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = 0.02 * (np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K))
    X = rng.standard_normal((n, D)); G = rng.standard_normal((n, D)); y = rng.standard_normal(n)
    Xrows = rng.standard_normal((n * nb, D)); yrows = rng.standard_normal(n * nb)
    eng.set_params(params)
    eng.condition_grad(X[:64], G[:64], alpha, Li, y=y[:64]); eng.condition(Xrows[:256], yrows[:256], alpha, Li)     # warm-up: allocations
    r = {'D': D, 'S': S, 'M': M, 'K': K, 'dtype': dt, 'points': n, 'rows_per_point': nb, 'points_per_chunk': npts, 'rows': n * nb}
    r['condition_grad_s'] = best(lambda: eng.condition_grad(X, G, alpha, Li, y=y))
    r['condition_same_rows_s'] = best(lambda: eng.condition(Xrows, yrows, alpha, Li))
    r['condition_grad_over_condition'] = r['condition_grad_s'] / r['condition_same_rows_s']
    eng.set_profiling(True)
    eng.condition_grad(X, G, alpha, Li, y=y)
    tot = {}
    for name, ms in eng.timings():
        tot[name] = tot.get(name, 0.0) + ms
    eng.set_profiling(False)
    nbytes = 8 * Kp * n * (1 + nb)                                 # fp64 in, fp64 out, all chunks
    k = {name: {'ms': ms} for name, ms in tot.items()}
    if 'gradobs_rows' in k:
        floor_ms = nbytes / (HBM_GBS * 1e9) * 1e3
        k['gradobs_rows'].update(bytes=nbytes, floor_ms=floor_ms, times_floor=tot['gradobs_rows'] / floor_ms)
    r['kernels'] = k
    eng.close()
    res[cfg if dt == 'f32' else cfg + '_f64'] = r
line = json.dumps({'condition_grad': res})
with open(OUT, 'w') as f:
    f.write(line + '\n')
print(line)
