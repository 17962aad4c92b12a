"""Time scfgp_select at the headline shape (D=64, S=32, M=1024), per dtype, pool size T and batch size m, and the loop it replaces
(m rounds of predict -> host argmax -> condition on one row, at m = 16 only).  Every (dtype, T) runs in a child process of its own
under a time limit; a child that fails or runs out of time ends the run.  One JSON line per case: wall times from host arrays to host
arrays (best of two calls; the first call of each kind, which allocates, is not timed), ms per pick from the difference of the two batch
sizes (the factor pass and the uploads cancel), and the sweep's achieved read rate T Kp sizeof(T) / (time per pick) -- a LOWER bound of
the sweep kernel's own rate, the small launches of a pick included -- next to the box probe's read-only stream.  The factors are a
synthetic posterior: the cost does not depend on their values.  Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/select_time.py --case f32 32768
Usage: python tools/select_time.py [--dtype f32,f64] [--limit SECONDS] [T ...]      (default: both; 300; 4096 32768 262144)
       python tools/select_time.py --case DTYPE T                                   (one case, in this process)"""
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
    Li = 0.02 * (np.tril(rng.standard_normal((K, K))) / np.sqrt(K) + np.eye(K))
    alpha = rng.standard_normal(K) / np.sqrt(K)
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    Kp = eng.dims()['Kp']
    eng.select(X[:256], Li, 4)                                     # first calls: allocations
    eng.predict(X[:256], alpha, Li)
    eng.condition(X[:1], np.zeros(1), alpha, Li)
    rec = {'D': D, 'S': S, 'M': M, 'K': K, 'dtype': dt, 'T': T, 'box_read_GBs': read_gbs}
    for m in MS:
        rec['select_m%d_s' % m] = best(lambda: eng.select(X, Li, m, return_std=True))
    per_pick = (rec['select_m%d_s' % MS[1]] - rec['select_m%d_s' % MS[0]]) / (MS[1] - MS[0])
    rec['ms_per_pick'] = 1e3 * per_pick
    rec['sweep_bytes'] = T * Kp * (4 if dt != 'f64' else 8)
    rec['sweep_GBs_lower_bound'] = rec['sweep_bytes'] / per_pick / 1e9
    rec['sweep_frac_of_box_read'] = rec['sweep_GBs_lower_bound'] / read_gbs

    def host_loop():
        a, L = alpha, Li
        taken = np.zeros(T, bool)
        for _ in range(MS[0]):
            _, sd = eng.predict(X, a, L)
            p = int(np.argmax(np.where(taken, -np.inf, sd)))
            taken[p] = True
            a, L = eng.condition(X[p:p + 1], np.zeros(1), a, L)
    rec['host_loop_m%d_s' % MS[0]] = best(host_loop, reps=1)
    rec['host_loop_ms_per_pick'] = 1e3 * rec['host_loop_m%d_s' % MS[0]] / MS[0]
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
