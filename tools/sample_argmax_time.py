"""Time scfgp_sample_argmax (per-sample maximisers, reduced in the epilogue of Phi* W) against the route it replaces, scfgp_sample
followed by numpy.argmax on the host, and next to scfgp_predict, at the headline shape (D=64, S=32, M=1024) and T = 10^6 pool rows, per
dtype and sample count.  Every figure is a host wall time around a call that ends in a device synchronise: one warm-up call of the same
shape, then `reps` timed calls, of which the median is reported (the spread is printed beside it).  The baseline's time includes the copy
of its T x nsamp fp64 block to pageable host memory (8 GB at nsamp = 1024) and the argmax over it; both routes return the same idx,
which the tool checks.  Writes a table to the output file and one JSON line to stdout.
Usage: python tools/sample_argmax_time.py [--T 1000000] [--reps 3] [--ns 16,256,1024] [--out profiles/sample_argmax_timing.txt]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scfgp_amd.engine import HipEngine, num_params


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


T = int(opt('--T', '1000000'))
REPS = int(opt('--reps', '3'))
NS = [int(a) for a in opt('--ns', '16,256,1024').split(',')]
OUT = opt('--out', os.path.join(ROOT, 'profiles', 'sample_argmax_timing.txt'))
D, S, M = 64, 32, 1024
K = 2 * (S + M)
rng = np.random.default_rng(7)
params = 0.1 * rng.standard_normal(num_params(D, S, M))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
Xs = rng.standard_normal((T, D))


def timed(f):
    """(median, min, max) wall seconds of REPS calls after one warm-up call, and the last result"""
    f()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
    return (float(np.median(ts)), min(ts), max(ts)), r


lines = ['scfgp_sample_argmax against scfgp_sample + numpy.argmax and scfgp_predict: D=%d S=%d M=%d (K=%d), T=%d pool rows' % (D, S, M, K, T),
         'host wall seconds per call (the call ends in a device synchronise); one warm-up, then median [min, max] of %d calls' % REPS,
         '%-5s %-6s %-28s %-28s %-28s %-8s' % ('dtype', 'nsamp', 'sample_argmax', 'sample + numpy.argmax', 'predict', 'ratio')]
res = {}
for dt in ('f32', 'f64'):
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    tp, _ = timed(lambda: eng.predict(Xs, alpha, Li))
    for ns in NS:
        ta, (idx, val) = timed(lambda: eng.sample_argmax(Xs, alpha, Li, ns, seed=1))

        def baseline():
            out = eng.sample(Xs, alpha, Li, ns, seed=1)
            i = np.argmax(out, axis=0)
            return i, out[i, np.arange(ns)]
        tb, (bidx, bval) = timed(baseline)
        same = bool(np.array_equal(idx, bidx) and np.array_equal(val, bval))
        fmt = lambda t: '%.4f [%.4f, %.4f]' % t
        lines.append('%-5s %-6d %-28s %-28s %-28s %-8.1f%s' % (dt, ns, fmt(ta), fmt(tb), fmt(tp), tb[0] / ta[0], '' if same else '  RESULTS DIFFER'))
        res['%s_ns%d' % (dt, ns)] = {'sample_argmax_s': ta[0], 'sample_plus_argmax_s': tb[0], 'predict_s': tp[0], 'ratio': tb[0] / ta[0],
                                     'same_result': same}
        print(lines[-1], flush=True)
    eng.close()
lines.append('ratio: (sample + numpy.argmax) / sample_argmax, medians')
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'T': T, 'reps': REPS, 'sample_argmax': res}))
