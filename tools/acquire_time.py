"""Time scfgp_acquire (UCB, EI, log-EI, and MES at n* = 16 / 256 / 1024) at the headline shape (D=64, S=32, M=1024) and T = 10^6 pool rows,
per dtype, next to scfgp_predict and against the route it replaces: scfgp_predict followed by a numpy / scipy evaluation of the same
formulas on the host (tests/acquire_ref.py).  With --grad also acquire with the input gradient against scfgp_predict_grad.  Every figure
is a host wall time around a call that ends in a device synchronise: one warm-up call of the same shape, then `reps` timed calls, of
which the median is reported (the spread is printed beside it).  The host evaluation of MES forms T x n* terms in numpy; --host-rows caps
the rows it is timed on (default 20000) and the figure is scaled to T, which the table says.  Writes a table to the output file and one
JSON line to stdout.
Usage: python tools/acquire_time.py [--T 1000000] [--reps 3] [--ns 16,256,1024] [--grad] [--host-rows 20000] [--out profiles/acquire_timing.txt]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scfgp_amd.engine import HipEngine, num_params
from tests import acquire_ref as A


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


T = int(opt('--T', '1000000'))
REPS = int(opt('--reps', '3'))
NS = [int(a) for a in opt('--ns', '16,256,1024').split(',')]
HOST_ROWS = int(opt('--host-rows', '20000'))
GRAD = '--grad' in sys.argv
OUT = opt('--out', os.path.join(ROOT, 'profiles', 'acquire_timing.txt'))
D, S, M = 64, 32, 1024
K = 2 * (S + M)
rng = np.random.default_rng(7)
params = 0.1 * rng.standard_normal(num_params(D, S, M))
alpha = rng.standard_normal(K) / np.sqrt(K)
Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
Xs = rng.standard_normal((T, D))


def timed(f, reps=REPS):
    """(median, min, max) wall seconds of `reps` calls after one warm-up call, and the last result"""
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t0)
    return (float(np.median(ts)), min(ts), max(ts)), r


fmt = lambda t: '%.4f [%.4f, %.4f]' % t
lines = ['scfgp_acquire next to scfgp_predict and against predict + a numpy / scipy host evaluation: D=%d S=%d M=%d (K=%d), T=%d pool rows'
         % (D, S, M, K, T),
         'host wall seconds per call (the call ends in a device synchronise); one warm-up, then median [min, max] of %d calls' % REPS,
         'host route: predict + tests/acquire_ref.py on the host; MES on %d rows, scaled to T' % min(HOST_ROWS, T),
         '%-5s %-10s %-28s %-28s %-12s %-28s' % ('dtype', 'kind', 'acquire', 'predict', 'host route', 'acquire + grad | predict_grad')]
res = {}
for dt in ('f32', 'f64'):
    eng = HipEngine(D, S, M, dtype=dt)
    eng.set_params(params)
    tp, (mu, sd) = timed(lambda: eng.predict(Xs, alpha, Li))
    mu = mu.ravel()
    best = float(np.median(mu))
    tg = timed(lambda: eng.predict_grad(Xs, alpha, Li))[0] if GRAD else None
    cases = [('ucb', dict(beta=2.0)), ('ei', dict(best=best)), ('logei', dict(best=best))]
    for ns in NS:
        cases.append(('mes%d' % ns, dict(fstar=eng.sample_argmax(Xs[:100000], alpha, Li, ns, seed=1)[1])))
    for name, kw in cases:
        kind = 'mes' if name.startswith('mes') else name
        ta, r = timed(lambda: eng.acquire(Xs, alpha, Li, kind, noise=True, **kw))
        rows = min(HOST_ROWS, T) if kind == 'mes' else T
        t0 = time.perf_counter(); ref = A.acquire(kind, mu[:rows], sd[:rows], **kw)[0]; th = (time.perf_counter() - t0) * T / rows
        err = A.kind_error(kind, r['acq'][:rows], ref, mu[:rows], sd[:rows], kw.get('beta'))
        tag = ''
        if GRAD:
            tag = fmt(timed(lambda: eng.acquire(Xs, alpha, Li, kind, noise=True, want=('acq', 'argmax', 'grad'), **kw))[0]) + ' | ' + fmt(tg)
        lines.append('%-5s %-10s %-28s %-28s %-12.2f %-28s' % (dt, name, fmt(ta), fmt(tp), tp[0] + th, tag))
        res['%s_%s' % (dt, name)] = {'acquire_s': ta[0], 'predict_s': tp[0], 'host_route_s': tp[0] + th, 'max_err_vs_host': err}
        print(lines[-1], flush=True)
    eng.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print(json.dumps({'D': D, 'S': S, 'M': M, 'K': K, 'T': T, 'reps': REPS, 'acquire': res}))
