"""Time scfgp_predict_gradcov next to scfgp_predict and scfgp_predict_grad (mean only) at equal point counts, at the headline shape
(D=64, S=32, M=1024) and at C5's (D=512, S=64, M=2048), fp32; and the call's own kernels (event times summed over the chunks) against
the larger of bytes / HBM rate and flops / peak.  Flop counts: T q K^2 for the triangular product C' = Psi Li^T, 2 T q^2 Kp for the
block Gram.  Prints one JSON line.
Usage: python tools/predict_gradcov_time.py [T_H [T_C5]]      (default: 8192 2048)"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from scfgp_amd.engine import HipEngine, num_params

PEAK_TFLOPS = {'f32': 157.3, 'f64': 78.6}                         # dense MFMA peaks (bench.py); the block Gram is fp64 MFMA in both
HBM_GBS = 8000.0
SHAPES = {'H': (64, 32, 1024), 'C5': (512, 64, 2048)}
Ts = [int(a) for a in sys.argv[1:]]
Ts = dict(zip(('H', 'C5'), Ts + [8192, 2048][len(Ts):]))


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


def kernel_rows(eng, T, D, S, M, dt):
    """event times of the call's kernels, summed over its chunks, and their floors"""
    q, K = min(D, S), 2 * (S + M)
    Kp = -(-K // 128) * 128
    ts = 4 if dt == 'f32' else 8
    tot = {}
    for name, ms in eng.timings():
        tot[name] = tot.get(name, 0.0) + ms
    rows = T * q
    floors = {
        'gradcov_dmu': (T * Kp * ts + T * D * 8, 2.0 * T * (S + M) * D, PEAK_TFLOPS[dt]),
        'gradfeat': (T * Kp * ts + rows * Kp * ts, 0.0, PEAK_TFLOPS[dt]),                     # reads Phi, writes Psi
        'gradcov_apply_c': (2 * rows * Kp * ts, float(rows) * K * K, PEAK_TFLOPS[dt]),        # reads Psi, writes C'
        'gradcov_block': (rows * Kp * ts + T * D * 8, 2.0 * rows * q * Kp, PEAK_TFLOPS['f64']),
    }
    out = {}
    for name, (nbytes, flops, peak) in floors.items():
        if name in tot:
            floor_ms = max(nbytes / (HBM_GBS * 1e9), flops / (peak * 1e12)) * 1e3
            out[name] = {'ms': tot[name], 'bytes': nbytes, 'flops': flops, 'floor_ms': floor_ms, 'times_floor': tot[name] / floor_ms}
    if 'gradcov_reduce' in tot:
        out['gradcov_reduce'] = {'ms': tot['gradcov_reduce']}
    return out


res = {}
rng = np.random.default_rng(7)
for cfg, (D, S, M) in SHAPES.items():
    T = Ts[cfg]
    K = 2 * (S + M)
    params = 0.1 * rng.standard_normal(num_params(D, S, M))
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    Xs = rng.standard_normal((T, D))
    dt = 'f32'
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    eng.predict_gradcov(Xs[:256], alpha, Li, want=('dmu', 'dvar', 'asub'))          # first call: allocations
    r = {'T': T, 'D': D, 'S': S, 'M': M, 'K': K, 'q': min(D, S), 'dtype': dt,
         'points_per_chunk': {'dvar': eng.gradcov_points_per_chunk(False), 'cov': eng.gradcov_points_per_chunk(True)}}
    r['predict_s'] = best(lambda: eng.predict(Xs, alpha, Li))
    r['grad_mean_s'] = best(lambda: eng.predict_grad(Xs, alpha, Li, want_std=False))
    r['gradcov_dvar_s'] = best(lambda: eng.predict_gradcov(Xs, alpha, Li, want=('dmu', 'dvar')))
    r['gradcov_asub_s'] = best(lambda: eng.predict_gradcov(Xs, alpha, Li, want=('dmu', 'dvar', 'asub')))
    eng.set_profiling(True)
    eng.predict_gradcov(Xs, alpha, Li, want=('dmu', 'dvar'))
    r['kernels_dvar'] = kernel_rows(eng, T, D, S, M, dt)
    eng.set_profiling(False)
    eng.close()
    res[cfg] = r
print(json.dumps({'predict_gradcov': res}))
