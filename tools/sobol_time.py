"""Time scfgp_sobol at the headline shape H (D=64, S=32, M=1024) in an fp32 context: the host wall time of one call (it ends in a
synchronise) for nw in {1, 256} with and without Vtot (without: no closed-set work, so no leave-one-out products), best of three after
a warm-up, and the event times of the call's kernels.  The pair kernel's fp64 rate counts 8 flops per (pair, set, column) over the
J (J + 1) / 2 pairs of the triangle doubled (the form's J^2 terms: the issue's count) and the sets the call forms.  Next to it predict on
1e6 rows, and how many pick-freeze base points n = rows / (D + 2) that one pass would buy.  Writes profiles/sobol_time_line.json and
prints it.
Usage: python tools/sobol_time.py [OUT.json]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.engine import HipEngine, num_params

D, S, M = 64, 32, 1024
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join('profiles', 'sobol_time_line.json')


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


J = S + M; K = 2 * J
rng = np.random.default_rng(7)
eng = HipEngine(D, S, M, dtype='f32')
eng.set_params(0.1 * rng.standard_normal(num_params(D, S, M)))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = 0.02 * (np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K))
kind = (np.arange(D) % 2).astype(np.int32)
p0 = np.where(kind == 1, 0.5, 0.0); p1 = np.where(kind == 1, 0.25, 1.0)
res = {'D': D, 'S': S, 'M': M, 'K': K, 'dtype': 'f32', 'contraction': 'vector pipe (fp64 FMA); the MFMA route was not built or measured'}
eng.sobol(kind, p0, p1, alpha)                                   # warm-up
for nw in (1, 256):
    W = alpha.reshape(-1, 1) if nw == 1 else eng.sample_weights(alpha, Li, nw, seed=1)
    for name, want in (('all', ('f0', 'V', 'Vmain', 'Vtot')), ('no_Vtot', ('f0', 'V', 'Vmain'))):
        r = {'wall_s': best(lambda: eng.sobol(kind, p0, p1, W, want=want))}
        eng.set_profiling(True)
        eng.sobol(kind, p0, p1, W, want=want)
        tot = {}
        for k, ms in eng.timings():
            tot[k] = tot.get(k, 0.0) + ms
        eng.set_profiling(False)
        r['kernels_ms'] = tot
        sets = 1 + D * (2 if 'Vtot' in want else 1)
        flops = 8.0 * sets * J * J * nw
        if tot.get('sobol_pairs'):
            r['pairs_gflops'] = flops / (tot['sobol_pairs'] * 1e-3) / 1e9
        res['nw%d_%s' % (nw, name)] = r
T = 1000000
X = rng.standard_normal((T, D))
eng.predict(X[:4096], alpha, Li)
res['predict_1e6_rows_s'] = best(lambda: eng.predict(X, alpha, Li))
res['pick_freeze_base_points_per_predict_pass'] = T // (D + 2)
eng.close()
line = json.dumps({'sobol': res})
with open(OUT, 'w') as f:
    f.write(line + '\n')
print(line)
