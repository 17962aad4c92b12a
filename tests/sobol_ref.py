"""numpy restatement of scfgp_sobol (include/scfgp_hip.h): closed-form Sobol variances of sample functions under a product measure,
with explicit leave-one-out products (every other factor multiplied out, no quotient), the abs-sum scales of the device bound, and
the mutants that the bound must reject.  Independent routes (tensor quadrature, pick-freeze Monte Carlo) are in test_sobol_ref.py."""
import numpy as np

from oracle import scfgp_oracle as O

EPS = 2.0 ** -52
MUTATIONS = ('no_conj', 'no_centre', 'swap_sets', 'no_half', 'no_s', 'full_width')


def phases(params, D, S, M):
    """Om (D x J), b (J), s: z_j = sum_e x_e Om[e][j] + b_j, phi = s [cos z | sin z]"""
    _, b, _, l_F, _, F, l_FC, FC = O.unpack_params(np.asarray(params, np.float64), D, S, M)
    return np.concatenate((l_F, F), 1), np.concatenate((l_FC, FC), 1)[0], float(np.exp(b) * np.sqrt(2.0 / M))


def psi(kind, p0, p1, om, mutate=None):
    """psi_d(om[d, ...]) for every input d: om has the inputs on axis 0"""
    sh = (-1,) + (1,) * (om.ndim - 1)
    kind = np.asarray(kind).reshape(sh); p0 = np.asarray(p0, np.float64).reshape(sh); p1 = np.asarray(p1, np.float64).reshape(sh)
    t = om * ((p1 - p0) if mutate == 'full_width' else 0.5 * (p1 - p0))
    with np.errstate(invalid='ignore', divide='ignore'):
        sinc = np.where(t == 0.0, 1.0, np.sin(t) / np.where(t == 0.0, 1.0, t))
    uni = np.exp(1j * om * (0.5 * (p0 + p1))) * sinc
    nor = np.exp(1j * om * p0 - 0.5 * (om * p1) ** 2)
    return np.where(kind == 1, nor, uni)


def loo(F, divide=False):
    """out[d] = prod_{e != d} F[e] along axis 0; divide: the quotient form that breaks at an exact zero"""
    if divide:
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.prod(F, 0)[None] / F
    out = np.empty_like(F)
    for d in range(F.shape[0]):
        out[d] = np.prod(np.delete(F, d, 0), 0) if F.shape[0] > 1 else 1.0
    return out


def sobol(params, D, S, M, kind, p0, p1, W, mutate=None, divide=False):
    """dict of f0, V (nw), Vmain, Vtot (nw x D), phibar (K) and the scales of the device bound: Sabs_all (nw), Sabs_main, Sabs_closed
    (nw x D), f0_abs (nw), a_sum (nw), s, E_abs (J), theta.  W (K, nw)."""
    Om, b, s = phases(params, D, S, M)
    J = S + M
    kind = np.zeros(D, int) if kind is None else np.asarray(kind)
    p0 = np.asarray(p0, np.float64); p1 = np.asarray(p1, np.float64)
    W = np.asarray(W, np.float64).reshape(2 * J, -1)
    a = (1.0 if mutate == 'no_s' else s) * (W[:J] - 1j * W[J:])                  # J x nw
    psi1 = psi(kind, p0, p1, Om, mutate)                                          # D x J
    eb1 = np.exp(1j * b)
    E = eb1 * np.prod(psi1, 0)
    Eld = eb1[None] * loo(psi1, divide)
    out = {'phibar': s * np.concatenate((E.real, E.imag)), 'f0': (a * E[:, None]).sum(0).real}
    nw = W.shape[1]
    Q = {u: np.zeros((nw,) + sh) for u, sh in (('all', ()), ('main', (D,)), ('closed', (D,)))}
    Sabs = {u: np.zeros_like(Q[u]) for u in Q}
    absa = np.abs(a)
    for sign in (1, -1):
        ck = (lambda x: x) if sign == 1 else np.conj
        Pp = psi(kind, p0, p1, Om[:, :, None] + sign * Om[:, None, :], mutate)    # D x J x J
        eb = np.exp(1j * (b[:, None] + sign * b[None, :]))
        cen = 0.0 if mutate == 'no_centre' else E[:, None] * ck(E)[None, :]
        C = {'all': eb * np.prod(Pp, 0) - cen,
             'main': Eld[:, :, None] * ck(Eld)[:, None, :] * Pp - cen,
             'closed': eb[None] * psi1[:, :, None] * ck(psi1)[:, None, :] * loo(Pp, divide) - cen}
        ak = a if (sign == 1 or mutate == 'no_conj') else np.conj(a)
        for u in Q:
            Q[u] += np.einsum('jw,kw,...jk->w...', a, ak, C[u]).real
            Sabs[u] += np.einsum('jw,kw,...jk->w...', absa, absa, np.abs(C[u]))
    half = 1.0 if mutate == 'no_half' else 0.5
    for u in Q:
        Q[u] *= half; Sabs[u] *= 0.5
    if mutate == 'swap_sets':
        Q['main'], Q['closed'] = Q['closed'], Q['main']
    out.update(V=Q['all'], Vmain=Q['main'], Vtot=Q['all'][:, None] - Q['closed'],
               Sabs_all=Sabs['all'], Sabs_main=Sabs['main'], Sabs_closed=Sabs['closed'],
               f0_abs=(absa * np.abs(E)[:, None]).sum(0), a_sum=absa.sum(0), s=s, E_abs=np.abs(E),
               theta=float(np.max(2.0 * np.abs(Om) * np.maximum(np.abs(p0), np.abs(p1))[:, None])))
    return out


def bounds(ref, D):
    """The device bound of every output: 1e-10 of the abs-sum of the terms plus the rounding of a coefficient, a
    difference of two products of at most 2 D + 2 factors of modulus <= 1 with a few eps of relative and eps theta of phase error
    each.  Vtot = V - Q_closed is a difference of two forms and gets the sum of their bounds."""
    r2 = (D + 2) * (1.0 + ref['theta']) * EPS
    var = lambda sabs: 1e-10 * sabs + 16 * r2 * (ref['a_sum'] ** 2).reshape((-1,) + (1,) * (sabs.ndim - 1))
    f0 = 1e-10 * ref['f0_abs'] + 8 * r2 * ref['a_sum']
    pb = 1e-10 * ref['s'] * ref['E_abs'] + 8 * r2 * ref['s']      # phibar: f0's bound per entry, a single a_j = s
    return {'V': var(ref['Sabs_all']), 'Vmain': var(ref['Sabs_main']), 'Vtot': var(ref['Sabs_all'])[:, None] + var(ref['Sabs_closed']),
            'f0': f0, 'phibar': np.concatenate((pb, pb))}


def worst_ratio(dev, ref, D):
    """{output: max |dev - ref| / bound} over the outputs that dev holds"""
    bd = bounds(ref, D)
    out = {}
    for k, b in bd.items():
        if dev.get(k) is None:
            continue
        err = np.abs(np.asarray(dev[k], np.float64).reshape(b.shape) - ref[k])
        with np.errstate(invalid='ignore', divide='ignore'):
            out[k] = float(np.max(np.where(err == 0.0, 0.0, err / b))) if np.all(np.isfinite(err)) else np.inf
    return out


def mixed_measure(D):
    """the parity measure: uniform on [0, 1] for even inputs, N(0.5, 0.25^2) for odd ones"""
    kind = (np.arange(D) % 2).astype(np.int32)
    return kind, np.where(kind == 1, 0.5, 0.0), np.where(kind == 1, 0.25, 1.0)


def parity_inputs(D, S, M):
    """params and W = [alpha | a perturbed alpha] of the parity tier, from gradcov_ref.synthetic"""
    from tests import gradcov_ref
    params, alpha, _ = gradcov_ref.synthetic(D, S, M)
    rng = np.random.default_rng(0x50B01 + D)
    return params, np.column_stack((alpha, alpha * (1.0 + 0.3 * rng.standard_normal(alpha.size))))
