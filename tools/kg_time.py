"""Time scfgp_acquire_kg at the headline shape (D=64, S=32, M=1024), T candidates against R reference rows with the default 31 nodes, per
dtype, next to scfgp_predict on the T rows, the cross form of scfgp_predict_cov at the same (T, R), and the route it replaces:
predict_cov + predict and the numpy reduction of the T x R matrix on the host (tests/kg_ref.py: node_table and bounds).  Every figure is
a host wall time around a call that ends in a device synchronise: one warm-up call of the same shape, then `reps` timed calls, of which
the median is reported with [min, max].  The host reduction forms J T x R arrays; --host-rows caps the candidate rows it is timed on
(default 1024) and the figure is scaled to T, which the record says.  Appends one JSON line to the output file and prints it.
Kernel times come from a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/kg_time.py --once
(--once: per dtype one warm-up and one timed call of scfgp_acquire_kg, nothing else, no file written).
Usage: python tools/kg_time.py [--T 16384] [--R 16384] [--J 31] [--reps 3] [--host-rows 1024] [--once] [--out profiles/kg_timing.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scfgp_amd.engine import HipEngine, num_params
from tests import kg_ref as G


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


T = int(opt('--T', '16384'))
R = int(opt('--R', '16384'))
J = int(opt('--J', '31'))
REPS = int(opt('--reps', '3'))
HOST_ROWS = min(int(opt('--host-rows', '1024')), T)
ONCE = '--once' in sys.argv
OUT = opt('--out', os.path.join(ROOT, 'profiles', 'kg_timing.json'))
D, S, M = 64, 32, 1024
K = 2 * (S + M)
rng = np.random.default_rng(7)
params = 0.1 * rng.standard_normal(num_params(D, S, M))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
Xc = rng.standard_normal((T, D))
Xr = rng.standard_normal((R, D))
z = np.linspace(-5.0, 5.0, J) if J % 2 else np.r_[np.linspace(-5.0, 0.0, J // 2 + 1), np.linspace(0.0, 5.0, J // 2 + 1)[1:-1]]


def timed(f, reps):
    """[median, min, max] wall seconds of `reps` calls after one warm-up call, and the last result"""
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
    return [float(np.median(ts)), min(ts), max(ts)], r


res = {}
for dt in ('f32', 'f64'):
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    tk, r = timed(lambda: eng.acquire_kg(Xc, alpha, Li, Xr=Xr, z=z, want=('kg', 'kg_hi', 'idx', 'val')), 1 if ONCE else REPS)
    rec = {'acquire_kg_s': tk}
    if not ONCE:
        rec['predict_s'], (mu_c, sd_c) = timed(lambda: eng.predict(Xc, alpha, Li), REPS)
        rec['predict_cov_cross_s'], cov = timed(lambda: eng.predict_cov(Xc, Li, Xb=Xr), REPS)
        mu_r = eng.predict(Xr, alpha, Li)[0].ravel()
        t0 = time.perf_counter()
        tab = G.node_table(G.offsets(mu_r), G.slopes(cov[:HOST_ROWS], sd_c[:HOST_ROWS]), z)
        kg, hi = G.bounds(*tab, z)
        th = (time.perf_counter() - t0) * T / HOST_ROWS
        rec['host_reduction_s'] = th
        rec['host_route_s'] = rec['predict_cov_cross_s'][0] + rec['predict_s'][0] + th
        scale = float(hi.max())
        rec['max_err_vs_host'] = float(max(np.abs(r['kg'][:HOST_ROWS] - kg).max(), np.abs(r['kg_hi'][:HOST_ROWS] - hi).max()) / scale)
        rec['max_gap_over_max_kg_hi'] = float((r['kg_hi'] - r['kg']).max() / r['kg_hi'].max())
        del cov
    res[dt] = rec
    print(dt, rec, flush=True)
    eng.close()
line = json.dumps({'tool': 'kg_time', 'D': D, 'S': S, 'M': M, 'K': K, 'T': T, 'R': R, 'J': J, 'reps': REPS, 'host_rows': HOST_ROWS,
                   'once': ONCE, 'acquire_kg': res})
if not ONCE:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, 'a') as f:
        f.write(line + '\n')
print(line)
