"""Time scfgp_select_iv at the headline shape (D=64, S=32, M=1024), per dtype, pool size T and batch size m, next to scfgp_select in the
same process.  Every (dtype, T) runs in a child process of its own under a time limit; a child that fails or runs out of time ends the
run.  One JSON line per case: wall times from host arrays to host arrays (best of two calls; the first call of each kind, which
allocates, is not timed), ms per pick from the difference of the two batch sizes (the factor pass, Q, the start values and the uploads
cancel), the same two columns of scfgp_select and the ratio of the two per-pick times, the sweep's achieved read rate T Kp sizeof(T) /
(time per pick) -- a LOWER bound, the small launches and the Kp x Kp GEMV of a pick included -- and the one-time cost of Q and the start
values: the m = 16 call minus scfgp_select's, with the 2 T Kp^2 flop of the start values' MFMA product over that time as a LOWER bound
of that kernel's rate (the reference is pool[::4], so Q's Gram runs over T / 4 rows).  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/select_iv_time.py --case f32 32768
Usage: python tools/select_iv_time.py [--dtype f32,f64] [--limit SECONDS] [T ...]      (default: both; 300; 4096 32768 262144)
       python tools/select_iv_time.py --case DTYPE T                                   (one case, in this process)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, S, M = 64, 32, 1024
K = 2 * (S + M)
MS = (16, 256)


def best(f, reps=2):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts)


def case(dt, T):
    import ctypes as C
    from scfgp_amd import _lib, synth
    from scfgp_amd.engine import HipEngine
    probe = (C.c_double * 7)()
    read_gbs = probe[6] if _lib.load().scfgp_box_probe(0, probe, 7) == 0 else float('nan')
    params = synth.make_params(11, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(7)
    X = synth.make_X(3, T, D)
    Xr = np.ascontiguousarray(X[::4]); wr = 0.5 + rng.random(len(Xr))
    Li = 0.02 * (np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K))
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    Kp = eng.dims()['Kp']
    eng.select(X[:256], Li, 4)                                     # first calls: allocations
    eng.select_iv(X[:256], Li, 4, Xr=Xr[:64], wr=wr[:64])
    rec = {'D': D, 'S': S, 'M': M, 'K': K, 'dtype': dt, 'T': T, 'R': len(Xr), 'box_read_GBs': read_gbs}
    for m in MS:
        rec['select_iv_m%d_s' % m] = best(lambda: eng.select_iv(X, Li, m, Xr=Xr, wr=wr, return_std=True))
        rec['select_m%d_s' % m] = best(lambda: eng.select(X, Li, m, return_std=True))
    per_pick = (rec['select_iv_m%d_s' % MS[1]] - rec['select_iv_m%d_s' % MS[0]]) / (MS[1] - MS[0])
    per_pick0 = (rec['select_m%d_s' % MS[1]] - rec['select_m%d_s' % MS[0]]) / (MS[1] - MS[0])
    rec['ms_per_pick'] = 1e3 * per_pick
    rec['select_ms_per_pick'] = 1e3 * per_pick0
    rec['per_pick_ratio_to_select'] = per_pick / per_pick0
    rec['sweep_bytes'] = T * Kp * (4 if dt != 'f64' else 8)
    rec['sweep_GBs_lower_bound'] = rec['sweep_bytes'] / per_pick / 1e9
    rec['sweep_frac_of_box_read'] = rec['sweep_GBs_lower_bound'] / read_gbs
    setup = rec['select_iv_m%d_s' % MS[0]] - MS[0] * per_pick - (rec['select_m%d_s' % MS[0]] - MS[0] * per_pick0)
    rec['q_and_start_values_s'] = setup
    rec['start_values_TFLOPs_lower_bound'] = 2.0 * T * Kp * Kp / setup / 1e12 if setup > 0 else float('nan')
    eng.close()
    print(json.dumps(rec), flush=True)


def main(argv):
    if argv[:1] == ['--case']:
        return case(argv[1], int(argv[2]))
    skip = set()

    def opt(name, default):
        if name in argv:
            skip.add(argv.index(name) + 1)
            return argv[argv.index(name) + 1]
        return default
    dtypes = opt('--dtype', 'f32,f64').split(',')
    limit = int(opt('--limit', '300'))
    Ts = [int(a) for i, a in enumerate(argv) if not a.startswith('-') and i not in skip] or [4096, 32768, 262144]
    for dt in dtypes:
        for T in Ts:
            # a fresh child per case, under its own time limit; the first failure ends the run
            r = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--case', dt, str(T)], cwd=ROOT)
            if r.returncode != 0:
                print(json.dumps({'dtype': dt, 'T': T, 'failed': r.returncode}), flush=True)
                return r.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]) or 0)
