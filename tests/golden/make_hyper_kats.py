"""
Regenerates tests/golden/hyper_kats.npz: the objective at parameter points far from (a, b, c) = (-1, 0, -1), with mpmath truths
(tests/hyper_ref.py: MpProblem, 60 digits, gradient by central differences) and, per point, what honest float64 rounding costs at that
conditioning (the float64 oracle on four row permutations of the same data, against the truth).  Needs mpmath, here only.

Shapes (N = 257: two 256-row blocks, one of a single row; M = 5 is no power of two, so sqrt(2 / M) is inexact):
    d3    (D, S, M) = (3, 2, 5)     dense projection, K = 14
    d20   (D, S, M) = (20, 2, 5)    Sp < Dp: the projection runs through the S columns.  The gradient keeps the dense form: the rank-S
                                    form (TZ / XU) needs Jp + round_up(S, 64) <= Kp, which no K below 130 meets, and K = 130 is out of
                                    mpmath's reach; tests/test_gpu_hyper_range.py takes those branches at (64, 2, 70) against the oracle
Points: the centre (-1, 0, -1), a star of single-axis moves from it and four corners in (a, c).
Per shape `<shape>/X, y, Xs, params` (the centre's vector; a point replaces its first three entries) and, stacked over the points,
    abc (n, 3), cost, cost_plain (n), grad (n, P), alpha (n, K), Li (n, K, K), mu, std (n, T), cond (n)   float64 roundings of the truths
    scale (n, P - 3)         the oracle's abs-sum scale of grad[3:] (the yardstick of the phase entries, whose truth is 0)
    ens (n, 8)               worst error of the four oracle runs: [cost (absolute), a, b, c (relative), l_F, r_F (norm-wise relative),
                             l_P, P (norm over the norm of the block's abs-sum scale)]
Grids: `grid/c`, `grid/kappa` (2, n) and `grid/b`, `grid/s5`, `grid/s300` (2, n): kappa over C_GRID + C_FAR and s = e^b sqrt(2 / M) over
B_GRID as double-double (high word, low word), so that a relative error of an ulp can be read against them.
Penalty: `pen/<D>_<S>_<M>/<case>`: R_PEN of tests/hyper_ref.py's edge rows with F = l_F r_F^T formed exactly.
cost_plain and std_plain are the truths with kappa replaced by float64's log(1 + e^c): what a library with that line computes, for the
vacuity guard of tests/test_gpu_hyper_range.py.
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
from scfgp_amd import synth          # noqa: E402
from tests import hyper_ref as H     # noqa: E402

N, T = 257, 5
SHAPES = {'d3': (3, 2, 5, 0x5CF6A003), 'd20': (20, 2, 5, 0x5CF6A020)}
CENTRE = (-1.0, 0.0, -1.0)
POINTS = ([CENTRE] + [(a, 0.0, -1.0) for a in (-7.0, -4.0, 2.0)] + [(-1.0, b, -1.0) for b in (-4.0, 4.0)]
          + [(-1.0, 0.0, c) for c in (-30.0, -20.0, -14.0, -10.0, 10.0, 30.0)]
          + [(a, 0.0, c) for a in (-7.0, 2.0) for c in (-30.0, 30.0)])
BLOCKS = ('cost', 'a', 'b', 'c', 'l_F', 'r_F', 'l_P', 'P')
PERM_SEEDS = (1, 2, 3, 4)


def shape_inputs(name):
    """(X, y (N, 1), Xs, params at the centre): a teacher's response + 0.1 noise, standardised"""
    from oracle import scfgp_oracle as O
    D, S, M, seed = SHAPES[name]
    X = synth.make_X(seed, N, D)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=CENTRE)
    teacher = synth.make_params(seed + 0x0101, D, S, M, abc=CENTRE)
    f = O.feature_map(X, teacher, D, S, M) @ synth.teacher_weights(seed + 0x0303, 2 * (S + M))
    y = synth.finish_targets(seed + 0x0404, f)
    return X, y.reshape(-1, 1), synth.make_X(seed + 0x0505, T, D), params


def block_slices(D, S, M):
    o = 3
    out = {}
    for k, n in (('l_F', D * S), ('r_F', M * S), ('l_P', S), ('P', M)):
        out[k] = slice(o, o + n); o += n
    return out


def block_errors(cost, grad, cost0, grad0, scale, D, S, M):
    """the eight figures of `ens` for one (cost, grad) against the truth (cost0, grad0)"""
    sl = block_slices(D, S, M)
    sc = np.concatenate((np.zeros(3), scale))
    d = np.asarray(grad, np.float64).ravel() - grad0
    out = [abs(float(cost) - cost0)] + [abs(d[i]) / abs(grad0[i]) for i in range(3)]
    out += [np.linalg.norm(d[sl[k]]) / np.linalg.norm(grad0[sl[k]]) for k in ('l_F', 'r_F')]
    out += [np.linalg.norm(d[sl[k]]) / np.linalg.norm(sc[sl[k]]) for k in ('l_P', 'P')]
    return np.array(out)


_PROBLEMS = {}


def _problem(name):
    if name not in _PROBLEMS:
        D, S, M, _ = SHAPES[name]
        X, y, Xs, params = shape_inputs(name)
        _PROBLEMS[name] = (H.MpProblem(X, y, S, M, Xs), params)
    return _PROBLEMS[name]


def _task(t):
    name, ip, i = t
    pr, params = _problem(name)
    p = params.copy(); p[:3] = POINTS[ip]
    mp = H._mp()
    if i >= 0:
        return t, float(pr.grad_entry(p, i))
    r = pr.evaluate(p, full=True)
    c = p[2]
    ratio = mp.mpf(float(np.log(1.0 + np.exp(c)))) / mp.log1p(mp.exp(mp.mpf(float(c))))       # kappa_plain / kappa
    # kappa enters the cost through d = kappa (v + 1) alone: T2 = sum (r^2 + v) / d + log(2 pi d)
    pq = pr.params(p)
    base = r['cost']
    plain = None
    if ratio > 0:
        # sum (r^2 + v) / d = N cost - the rest, the rest does not depend on kappa: evaluate at c' with kappa(c') = kappa_plain instead
        cp = mp.log(mp.expm1(ratio * mp.log1p(mp.exp(pq[2]))))
        pq[2] = cp
        plain = pr.evaluate(pq)
    return t, dict(cost=float(base), cost_plain=float(plain) if plain is not None else np.inf, alpha=H.to_f64(r['alpha']),
                   Li=H.to_f64(r['Li']), mu=H.to_f64(r['mu']), std=H.to_f64(r['std']), cond=float(H.mp_cond(r['A'])),
                   std_plain=H.to_f64(r['std']) * float(mp.sqrt(ratio)))


def dd(x):
    """(high, low) float64 words of an mpf"""
    hi = float(x)
    return hi, float(x - H._mp().mpf(hi))


PEN_SHAPES_GPU = [(3, 2, 5), (2, 70, 300), (64, 2, 70)]


def grids_and_penalties():
    mp = H._mp()
    out = {}
    cs = np.concatenate((H.C_GRID, H.C_FAR))
    out['grid/c'] = cs
    out['grid/kappa'] = np.array([dd(H.mp_scalars(0.0, 0.0, c, 5)['kappa']) for c in cs]).T
    out['grid/b'] = H.B_GRID
    for M in H.M_GRID:
        out['grid/s%d' % M] = np.array([dd(H.mp_scalars(0.0, b, 0.0, M)['s']) for b in H.B_GRID]).T
    for D, S, M in PEN_SHAPES_GPU:
        for case in H.EDGE_CASES:
            l_F, r_F = H.edge_factors(case, D, S, M)
            lm, rm = H._mp_rows(l_F), H._mp_rows(r_F)
            F = [[mp.fdot(lm[d], rm[m]) for m in range(M)] for d in range(D)]
            out['pen/%d_%d_%d/%s' % (D, S, M, case)] = float(H.mp_penalty(lm, F)[0])
    return out


def main():
    from oracle import scfgp_oracle as O
    tasks = []
    for name, (D, S, M, seed) in SHAPES.items():
        P = O.num_params(D, S, M)
        for ip in range(len(POINTS)):
            tasks += [(name, ip, i) for i in range(-1, P)]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        res = dict(pool.imap_unordered(_task, tasks, chunksize=4))
    out = grids_and_penalties()
    for name, (D, S, M, seed) in SHAPES.items():
        X, y, Xs, params = shape_inputs(name)
        P = O.num_params(D, S, M)
        out.update({name + '/X': X, name + '/y': y, name + '/Xs': Xs, name + '/params': params})
        cols = dict((k, []) for k in ('abc', 'cost', 'cost_plain', 'grad', 'alpha', 'Li', 'mu', 'std', 'std_plain', 'cond', 'scale', 'ens'))
        for ip, abc in enumerate(POINTS):
            r = res[(name, ip, -1)]
            grad = np.array([res[(name, ip, i)] for i in range(P)])
            p = params.copy(); p[:3] = abc
            scale = O.value_and_grad(X, y, p, S, M, with_scale=True)[4]
            ens = np.zeros(len(BLOCKS))
            for ps in PERM_SEEDS:
                perm = np.random.default_rng(ps).permutation(N)
                c1, g1 = O.value_and_grad(np.ascontiguousarray(X[perm]), np.ascontiguousarray(y[perm]), p, S, M)[:2]
                ens = np.maximum(ens, block_errors(c1, g1, r['cost'], grad, scale, D, S, M))
            print('%s %-18s cost %+.6e cond %.1e ens %s' % (name, abc, r['cost'], r['cond'], ' '.join('%.1e' % v for v in ens)), flush=True)
            cols['abc'].append(abc); cols['grad'].append(grad); cols['scale'].append(scale); cols['ens'].append(ens)
            for k in ('cost', 'cost_plain', 'alpha', 'Li', 'mu', 'std', 'std_plain', 'cond'):
                cols[k].append(r[k])
        for k, v in cols.items():
            out['%s/%s' % (name, k)] = np.array(v, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, 'hyper_kats.npz'), **out)


if __name__ == '__main__':
    main()
