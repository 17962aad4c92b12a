"""Time scfgp_select_qei (greedy Monte-Carlo batch expected improvement over a pool) next to scfgp_sample_argmax, which runs the same
product Phi* W over the same rows without storing it, at D=64, S=32, M=992 (K=2048), fp32, T = 10^6 pool rows, nsamp = 256, m = 16; and
against the route it replaces, scfgp_sample to the host followed by the numpy greedy of tests/select_qei_ref.py, at a pool size where
that route finishes (--T-host, default 131072: a 268 MB block).  Every figure is a host wall time from host arrays to host arrays around
a call that ends in a device synchronise: one warm-up call of the same shape, then `reps` timed calls, median [min, max].  The time per
pick is the difference of two batch sizes (m and 3 m: the product, the uploads and the first sweep cancel), and the sweep's achieved
read rate T nsamp 8 / (time per pick) is a LOWER bound of the sweep kernel's own rate, the commit launch of a pick included; it is
printed next to the box probe's read-only stream figure (scfgp_box_probe out[6]) of the same run.  The factors are a synthetic
posterior: the cost does not depend on their values.  Writes the lines to the output file and one JSON line to stdout.
Usage: python tools/select_qei_time.py [--T 1000000] [--T-host 131072] [--ns 256] [--m 16] [--reps 3] [--dtype f32]
                                       [--out profiles/select_qei_timing.txt]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scfgp_amd import _lib, synth
from scfgp_amd.engine import HipEngine
from tests import select_qei_ref as Q


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


T = int(opt('--T', '1000000'))
TH = int(opt('--T-host', '131072'))
NS = int(opt('--ns', '256'))
MP = int(opt('--m', '16'))
REPS = int(opt('--reps', '3'))
DT = opt('--dtype', 'f32')
OUT = opt('--out', os.path.join(ROOT, 'profiles', 'select_qei_timing.txt'))
D, S, M = 64, 32, 992
K = 2 * (S + M)


def timed(f):
    """(median, min, max) wall seconds of REPS calls after one warm-up call, and the last result"""
    f()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
    return (float(np.median(ts)), min(ts), max(ts)), r


probe = (C.c_double * 7)()
read_gbs = probe[6] if _lib.load().scfgp_box_probe(0, probe, 7) == 0 else float('nan')
params = synth.make_params(11, D, S, M, abc=(-1.0, 0.0, -1.0))
rng = np.random.default_rng(7)
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
Xs = synth.make_X(3, T, D)
eng = HipEngine(D, S, M, dtype=DT)
eng.set_params(params)
fmt = lambda t: '%.4f [%.4f, %.4f]' % t
lines = ['scfgp_select_qei next to scfgp_sample_argmax and against scfgp_sample + the numpy greedy: D=%d S=%d M=%d (K=%d), %s, nsamp=%d' % (
             D, S, M, K, DT, NS),
         'host wall seconds per call (the call ends in a device synchronise); one warm-up, then median [min, max] of %d calls' % REPS]

# the incumbent: the median of the per-sample maxima over the first rows, so that the picks have something to gain
best = float(np.median(eng.sample(Xs[:4096], alpha, Li, NS, seed=1).max(axis=0)))
ta, _ = timed(lambda: eng.sample_argmax(Xs, alpha, Li, NS, seed=1))
t1, r1 = timed(lambda: eng.select_qei(Xs, alpha, Li, MP, NS, best, seed=1))
t3, r3 = timed(lambda: eng.select_qei(Xs, alpha, Li, 3 * MP, NS, best, seed=1))
per_pick = (t3[0] - t1[0]) / (2 * MP)
sweep_bytes = T * NS * 8
sweep_gbs = sweep_bytes / per_pick / 1e9
prefix = bool(np.array_equal(r1[0], r3[0][:MP]) and np.array_equal(r1[1], r3[1][:MP]))
lines += ['T=%d:  sample_argmax %s   select_qei m=%d %s   m=%d %s' % (T, fmt(ta), MP, fmt(t1), 3 * MP, fmt(t3)),
          'per pick %.3f ms: one sweep over F (%.3f GB) and one commit; sweep read rate >= %.0f GB/s; box probe read-only stream %.0f GB/s '
          '(ratio %.2f)%s' % (1e3 * per_pick, sweep_bytes / 1e9, sweep_gbs, read_gbs, sweep_gbs / read_gbs, '' if prefix else '  PREFIX DIFFERS'),
          'gains of the m=%d call: %s' % (MP, np.array2string(r1[1], precision=4))]
print('\n'.join(lines[2:]), flush=True)

Xh = Xs[:TH]
td, rd = timed(lambda: eng.select_qei(Xh, alpha, Li, MP, NS, best, seed=1))


def host_route():
    F = eng.sample(Xh, alpha, Li, NS, seed=1)
    t0 = time.perf_counter()
    out = Q.greedy(F, MP, best)
    return out, time.perf_counter() - t0


th, (rh, greedy_s) = timed(host_route)
same = bool(np.array_equal(rd[0], rh[0]))
lines += ['T=%d:  select_qei m=%d %s   sample + numpy greedy %s (the greedy alone %.3f)   ratio %.1f%s' % (
    TH, MP, fmt(td), fmt(th), greedy_s, th[0] / td[0], '' if same else '  PICKS DIFFER')]
print(lines[-1], flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'dtype': DT, 'T': T, 'nsamp': NS, 'm': MP, 'reps': REPS, 'sample_argmax_s': ta[0],
                  'select_qei_s': t1[0], 'select_qei_3m_s': t3[0], 'ms_per_pick': 1e3 * per_pick, 'sweep_GBs_lower_bound': sweep_gbs,
                  'box_read_GBs': read_gbs, 'T_host': TH, 'select_qei_host_size_s': td[0], 'sample_plus_numpy_greedy_s': th[0],
                  'same_picks': same, 'prefix': prefix}))
