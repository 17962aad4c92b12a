"""Time scfgp_predict_pd at the headline shape (D=64, S=32, M=1024), fp32, over a pool of T rows for ndim dimensions and G grid values:
  1. the call with pd + sd (host clock around the call, which ends in a device synchronise; best of 3 after a warm-up call),
  2. predict on the same T rows,
  3. predict on a slice of the T G ndim expanded rows (every (dimension, grid value) copy of the pool's first T / (G ndim) rows), scaled
     up by the row count and labelled EXTRAPOLATED (the only route to the ICE values without this entry point; it gives no PD
     uncertainty at all),
  4. on one chunk of 32 768 rows in the same process, from the library's own event timers: the sums kernel over all ndim dimensions
     against ndim times one feature-map launch -- the floor of the alternative that materialises Phi0 per dimension and reduces it.
Also the ICE path of one chunk (feature map and product per dimension).  Writes one JSON line to stdout and, with --out, to that file.
Usage: python tools/pd_time.py [--T 1000000] [--ndim 64] [--G 32] [--out profiles/pd_time_line.json]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.engine import HipEngine, num_params


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts), ts


def scopes(eng):
    tot, cnt = {}, {}
    for name, ms in eng.timings():
        tot[name] = tot.get(name, 0.0) + ms
        cnt[name] = cnt.get(name, 0) + 1
    return tot, cnt


D, S, M = 64, 32, 1024
T, ndim, G = arg('--T', 1000000), arg('--ndim', 64), arg('--G', 32)
CH = 32768
K = 2 * (S + M)
rng = np.random.default_rng(7)
params = 0.1 * rng.standard_normal(num_params(D, S, M))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
Xs = rng.standard_normal((T, D))
w = 0.25 + rng.uniform(0, 1, T)
dims = list(range(ndim))
grid = np.tile(np.linspace(-2.0, 2.0, G), (ndim, 1))
eng = HipEngine(D, S, M, dtype='f32')
eng.set_params(params)
n1 = min(T, CH)
eng.predict_pd(Xs[:n1], alpha, Li, dims, grid, w=w[:n1], want=('pd', 'sd', 'ice'))        # first call: allocations, code objects
eng.predict(Xs[:n1], alpha, Li)
r = {'D': D, 'S': S, 'M': M, 'K': K, 'dtype': 'f32', 'T': T, 'ndim': ndim, 'G': G}
r['pd_sd_s'], r['pd_sd_all_s'] = best(lambda: eng.predict_pd(Xs, alpha, Li, dims, grid, w=w))
r['predict_T_rows_s'], r['predict_T_rows_all_s'] = best(lambda: eng.predict(Xs, alpha, Li))
# a slice of the expanded rows: every (dimension, grid value) copy of the first rows of the pool, about as many rows as the pool has
n0 = max(1, T // (G * ndim))
Xe = np.repeat(Xs[None, :n0, :], ndim * G, 0).reshape(ndim, G, n0, D)
for a, d in enumerate(dims):
    Xe[a, :, :, d] = grid[a][:, None]
Xe = np.ascontiguousarray(Xe.reshape(-1, D))
r['expanded_rows'] = T * G * ndim
r['expanded_slice_rows'] = len(Xe)
r['predict_expanded_slice_s'], r['predict_expanded_slice_all_s'] = best(lambda: eng.predict(Xe, alpha, Li))
r['predict_expanded_rows_s_EXTRAPOLATED'] = r['predict_expanded_slice_s'] * r['expanded_rows'] / len(Xe)
del Xe
# one chunk, event timers on
eng.set_profiling(True)
eng.predict_pd(Xs[:n1], alpha, Li, dims, grid, w=w[:n1])
tot, cnt = scopes(eng)
r['chunk_rows'] = n1
r['chunk_pd_sums_ms'] = tot.get('pd_sums')
r['chunk_pd_sums_launches'] = cnt.get('pd_sums')
r['chunk_pd_curves_ms'] = tot.get('pd_curves')
nd_ice = min(ndim, 16)                                            # HipEngine.timings() returns the first 64 records: two per dimension here
eng.predict_pd(Xs[:n1], alpha, Li, dims[:nd_ice], grid[:nd_ice], want=('ice',))
tot, cnt = scopes(eng)
r['chunk_ice_dimensions_timed'] = nd_ice
fm = tot['pd_ice_featuremap'] / cnt['pd_ice_featuremap']
r['chunk_featuremap_launch_ms'] = fm
r['chunk_ndim_featuremap_launches_ms'] = fm * ndim
r['chunk_ice_product_ms_per_dimension'] = tot['pd_ice_product'] / cnt['pd_ice_product']
r['sums_kernel_over_featuremap_floor'] = r['chunk_pd_sums_ms'] / (fm * ndim)
eng.set_profiling(False)
eng.close()
line = json.dumps({'predict_pd': r})
print(line)
if '--out' in sys.argv:
    with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
        f.write(line + '\n')
