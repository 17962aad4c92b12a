"""
GPU parity tests proper: the HIP path, called through the C ABI (ctypes) behind the
reference's function-triple interface, against
  (1) the reference's own artifact (Theano-computed Li / alpha / COST),
  (2) the committed oracle KATs (cost, gradient, alpha, Li, predictive mean / sigma),
  (3) the CPU oracle on the same seeded inputs,
  (4) size-independent properties at BASELINE.json's full sizes.
Tolerances: north_star asks 1e-5 relative in fp64; the fp64 path is asserted at 1e-9 or
tighter.  fp32 mode (SCFGP_F32) is asserted at |dcost| <= 1e-5 max(1,|cost|) and per-block
gradient norms <= 1e-3.
"""
import os

import numpy as np
import pytest

from oracle import scfgp_oracle as O
from scfgp_amd import synth
from tests import parity as PB
from tests.golden.make_oracle_kats import CASES, case_inputs

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def grad_blocks(g, D, S, M):
    o = 3 + D * S
    return g[:3], g[3:o], g[o:o + M * S]


# ---------------------------------------------------------------------------------------------
def test_artifact_kat_through_the_triple():
    """train_func on the reference's 400-row Boston split reproduces Theano's outputs."""
    from scfgp_amd.funcs import CompiledFuncs
    z = np.load(os.path.join(GOLD, 'artifact_kat.npz'))
    S, M, D = int(z['S']), int(z['M']), int(z['D'])
    cf = CompiledFuncs(D, S, M, z['params'], 'adam', {'learning_rate': 0.01})
    train_func, train_iter_func, pred_func = cf.triple()
    cost, alpha, Li = train_func(z['X'], z['y'])
    assert isinstance(cost, np.ndarray) and cost.ndim == 0 and alpha.shape == (2 * (S + M), 1)
    assert abs(float(cost) - float(z['cost'])) < 1e-11 * abs(float(z['cost']))
    assert rel(Li, z['Li']) < 1e-10 and rel(alpha, z['alpha']) < 1e-9
    assert np.all(np.triu(Li, 1) == 0)


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_kats_fp64(name):
    from scfgp_amd.funcs import CompiledFuncs
    z = np.load(os.path.join(GOLD, 'oracle_kats.npz'))
    N, D, S, M, T, seed = CASES[name]
    X, y, params, Xs = case_inputs(name)
    cf = CompiledFuncs(D, S, M, params.copy(), 'adam', {'learning_rate': 0.01, 'beta2': 0.999})
    train_func, train_iter_func, pred_func = cf.triple()
    cost, grad, alpha, Li = cf.value_and_grad(X, y)
    assert abs(float(cost) - float(z[name + '/cost'])) < 1e-10 * abs(float(cost))
    assert rel(grad, z[name + '/grad']) < 1e-8
    gb, zb = grad_blocks(grad, D, S, M), grad_blocks(z[name + '/grad'], D, S, M)
    assert all(rel(u, v) < 1e-8 for u, v in zip(gb, zb))
    assert rel(alpha, z[name + '/alpha']) < 1e-8
    if name + '/Li' in z.files:
        assert rel(Li, z[name + '/Li']) < 1e-9
    else:
        assert rel(Li[z[name + '/Li_rows']], z[name + '/Li_sample']) < 1e-9
        assert abs(np.linalg.norm(Li) - float(z[name + '/Li_fro'])) < 1e-9 * float(z[name + '/Li_fro'])
    mu, sd = pred_func(Xs, alpha, Li)
    assert mu.shape == (T, 1) and sd.shape == (T,)
    assert rel(mu, z[name + '/mu']) < 1e-8 and rel(sd, z[name + '/std']) < 1e-9
    ref = PB.oracle_all(X, y, params, S, M, Xs)
    r = PB.check_all((cost, grad, alpha, Li), ref, D, S, M, 'f64')
    r['predict'] = PB.check_predict(mu, sd, ref['mu'], ref['std'], 'f64')
    print('\n%s f64 blocks: %s' % (name, PB.fmt(r)))
    # train_iter_func: outputs at the PRE-update parameters, then the vector moves
    c2, a2, L2 = train_iter_func(X, y)
    assert float(c2) == float(cost) and np.array_equal(a2, alpha)
    assert not np.array_equal(cf.params.get_value(), params)
    c3, _, _ = train_func(X, y)
    assert float(c3) != float(cost)


@pytest.mark.parametrize('mode', ['f32'])
@pytest.mark.parametrize('name', ['artifact_shape', 'c1_boston_shape', 'c2_small_n'])
def test_oracle_kats_fp32_mode(name, mode):
    from scfgp_amd.engine import HipEngine
    z = np.load(os.path.join(GOLD, 'oracle_kats.npz'))
    N, D, S, M, T, seed = CASES[name]
    X, y, params, Xs = case_inputs(name)
    eng = HipEngine(D, S, M, dtype=mode); eng.set_params(params); eng.set_data(X, y)
    cost, grad, alpha, Li = eng.eval(want_grad=True)
    c0 = float(z[name + '/cost'])
    assert abs(float(cost) - c0) < 1e-5 * max(1.0, abs(c0))
    for u, v in zip(grad_blocks(grad, D, S, M), grad_blocks(z[name + '/grad'], D, S, M)):
        assert rel(u, v) < 1e-3
    assert rel(alpha, z[name + '/alpha']) < 1e-3
    mu, sd = eng.predict(Xs, z[name + '/alpha'], Li)
    assert rel(mu, z[name + '/mu']) < 1e-4 and rel(sd, z[name + '/std']) < 1e-4
    r = PB.check_all((cost, grad, alpha, Li), PB.oracle_all(X, y, params, S, M), D, S, M, mode)
    mu0, sd0 = O.predict(Xs, z[name + '/alpha'], Li, params, S, M)
    r['predict'] = PB.check_predict(mu, sd, mu0, sd0, mode)
    print('\n%s %s blocks: %s' % (name, mode, PB.fmt(r)))
    eng.close()


# ---------------------------------------------------------------------------------------------
def test_error_behaviour_matches_reference():
    from scfgp_amd.funcs import CompiledFuncs
    N, D, S, M, T, seed = CASES['tiny_257x5']
    X, y, params, Xs = case_inputs('tiny_257x5')
    cf = CompiledFuncs(D, S, M, params.copy())
    tf, tif, pf = cf.triple()
    with pytest.raises(TypeError):                 # dmatrix rejects float32 (SCFGP.py:95)
        tf(X.astype(np.float32), y)
    with pytest.raises(TypeError):                 # ... and 1-d targets
        tf(X, y.ravel())
    bad = params.copy(); bad[3] = np.nan
    cf.params.set_value(bad)
    with pytest.raises(np.linalg.LinAlgError):     # Cholesky failure (SCFGP.py:106)
        tf(X, y)
    with pytest.raises(ValueError):
        CompiledFuncs(D, S, M, params, algo='norm_constraint')


def test_resident_data_is_re_uploaded_after_invalidate():
    """X, y stay on the GPU while the caller keeps passing the same arrays; an in-place edit needs invalidate()."""
    from scfgp_amd.funcs import CompiledFuncs
    name = 'tiny_257x5'
    N, D, S, M, T, seed = CASES[name]
    X, y, params, _ = case_inputs(name)
    cf = CompiledFuncs(D, S, M, params.copy())
    c0 = float(cf.train_func(X, y)[0])
    assert float(cf.train_func(X, y)[0]) == c0                      # second call: resident, same result
    y[1::2] += 0.25                                                  # in-place edit (hits sampled elements or not)
    cf.invalidate()
    c1 = float(cf.train_func(X, y)[0])
    c_ref = O.forward(X, y, params, S, M)[0]
    assert abs(c1 - c_ref) < 1e-10 * abs(c_ref) and c1 != c0


def test_minibatches_of_different_sizes():
    """N is per call (batch size enters 2(N-M)a and /N, SCFGP.py:126,128)."""
    from scfgp_amd.funcs import CompiledFuncs
    name = 'kin8nm_like'
    N, D, S, M, T, seed = CASES[name]
    X, y, params, _ = case_inputs(name)
    cf = CompiledFuncs(D, S, M, params.copy())
    for lo, hi in [(0, 150), (150, 1000), (37, 300), (0, 1000)]:
        Xb, yb = np.ascontiguousarray(X[lo:hi]), np.ascontiguousarray(y[lo:hi])
        c, g, a, L = cf.value_and_grad(Xb, yb)
        c0, g0, a0, L0 = O.value_and_grad(Xb, yb, params, S, M)
        assert abs(float(c) - c0) < 1e-10 * abs(c0) and rel(g, g0) < 1e-7 and rel(a, a0) < 1e-7
        PB.oracle_check((c, g, a, L), Xb, yb, params, S, M, 'f64', label='minibatch')


@pytest.mark.parametrize('N,D,S,M', [(1, 1, 2, 2), (3, 2, 2, 3), (255, 3, 2, 5), (513, 70, 5, 60),
                                     (300, 200, 3, 9), (1000, 5, 64, 3), (2000, 7, 31, 33),
                                     (700, 4, 8, 120), (900, 6, 10, 150)])      # K = 256: no Gram strip; K = 320: strip
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_ragged_and_degenerate_shapes(N, D, S, M, dtype):
    """Sizes that are not multiples of any tile: padding rows/columns must never leak."""
    from scfgp_amd.engine import HipEngine
    rng = np.random.default_rng(N * 7 + D)
    X = rng.random((N, D)); y = rng.standard_normal((N, 1))
    params = O.init_params(D, S, M, rng)
    params[0] = -0.5; params[1] = 0.1; params[2] = -0.7; params[3:3 + D * S] *= 0.7
    Xs = rng.random((17, D))
    eng = HipEngine(D, S, M, dtype=dtype); eng.set_params(params); eng.set_data(X, y)
    cost, grad, alpha, Li = eng.eval(want_grad=True)
    c0, g0, a0, L0 = O.value_and_grad(X, y, params, S, M)
    tol = 1e-8 if dtype == 'f64' else 2e-3
    ftol = tol if dtype == 'f64' else 2e-2      # alpha, Li carry cond(A) times the fp32 Gram error
    assert abs(float(cost) - c0) < (1e-10 if dtype == 'f64' else 2e-5) * max(1.0, abs(c0))
    assert rel(grad, g0) < tol and rel(alpha, a0) < ftol and rel(Li, L0) < ftol
    PB.oracle_check((cost, grad, alpha, Li), X, y, params, S, M, dtype, alpha_li=dtype == 'f64', label='ragged')
    mu, sd = eng.predict(Xs, a0, L0)
    mu0, sd0 = O.predict(Xs, a0, L0, params, S, M)
    assert rel(mu, mu0) < tol and rel(sd, sd0) < tol
    PB.check_predict(mu, sd, mu0, sd0, dtype)
    # a second, smaller data set through the same context (capacity is kept, padding rewritten)
    n2 = max(1, N // 3)
    c2, g2, _, _ = eng.eval(np.ascontiguousarray(X[:n2]), np.ascontiguousarray(y[:n2]), want_grad=True)
    c3, g3, _, _ = O.value_and_grad(X[:n2], y[:n2], params, S, M)
    assert abs(float(c2) - c3) < (1e-10 if dtype == 'f64' else 2e-5) * max(1.0, abs(c3)) and rel(g2, g3) < tol
    eng.close()


# ---------------------------------------------------------------------------------------------
def _synthetic(N, D, S, M, seed):
    X = synth.make_X(seed, N, D)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    return X, params


def _teacher_targets(eng, X, D, S, M, seed):
    """y = standardise(Phi(X; teacher) w + 0.1 eps) with Phi.w computed by the HIP predict path."""
    K = 2 * (S + M)
    teacher = synth.make_params(seed + 0x0101, D, S, M, abc=(-1.0, 0.0, -1.0))
    eng.set_params(teacher)
    f, _ = eng.predict(X, synth.teacher_weights(seed + 0x0303, K), np.eye(K))
    return synth.finish_targets(seed + 0x0404, f).reshape(-1, 1)


def test_c2_full_size_against_oracle_and_invariances():
    """BASELINE config 2 (N=1e5, D=32, S=16, M=256, fp64) at full size."""
    from scfgp_amd.engine import HipEngine
    N, D, S, M, seed = 100000, 32, 16, 256, 0x5CF60002
    J = S + M; K = 2 * J
    X, params = _synthetic(N, D, S, M, seed)
    eng = HipEngine(D, S, M, dtype='f64')
    y = _teacher_targets(eng, X, D, S, M, seed)
    eng.set_params(params); eng.set_data(X, y)
    cost, grad, alpha, Li = eng.eval(want_grad=True)
    c0, g0, a0, L0 = O.value_and_grad(X, y, params, S, M, chunk=8192)
    assert abs(float(cost) - c0) < 1e-10 * abs(c0)
    assert rel(grad, g0) < 1e-8 and rel(alpha, a0) < 1e-8 and rel(Li, L0) < 1e-9
    # phase invariance: d cost / d phases == 0, cost unchanged under a phase shift
    assert np.abs(grad[-J:]).max() < 1e-9 * np.abs(grad).max()
    p2 = params.copy(); p2[-J:] += np.linspace(0.0, 3.0, J)
    eng.set_params(p2)
    c2, g2, _, _ = eng.eval(want_grad=True)
    assert abs(float(c2) - float(cost)) < 1e-9 * abs(float(cost)) and rel(g2[:-J], grad[:-J]) < 1e-6
    # row permutation invariance
    perm = np.random.default_rng(0).permutation(N)
    eng.set_params(params); eng.set_data(np.ascontiguousarray(X[perm]), np.ascontiguousarray(y[perm]))
    c3, g3, a3, _ = eng.eval(want_grad=True)
    assert abs(float(c3) - float(cost)) < 1e-11 * abs(float(cost)) and rel(g3, grad) < 1e-8 and rel(a3, alpha) < 1e-8
    # pair identity on the Gram diagonal: G[j,j] + G[J+j,J+j] = N s^2
    eng.pass1()
    Kp = eng.dims()['Kp']
    G = eng.debug_read('G', (Kp * Kp,)).reshape(Kp, Kp)
    s2 = np.exp(2 * params[1]) * 2.0 / M
    assert np.allclose(np.diag(G)[:J] + np.diag(G)[J:K], N * s2, rtol=1e-12)
    eng.close()


def test_headline_size_fp32_properties():
    """Headline workload (N=1e6, D=64, S=32, M=1024 => K=2112) in fp32 mode: properties only
    (the oracle would need minutes here)."""
    from scfgp_amd.engine import HipEngine
    N, D, S, M, seed = 1000000, 64, 32, 1024, 0x5CF600FF
    J = S + M; K = 2 * J
    X, params = _synthetic(N, D, S, M, seed)
    eng = HipEngine(D, S, M, dtype='f32')
    y = _teacher_targets(eng, X, D, S, M, seed)
    eng.set_params(params); eng.set_data(X, y)
    cost, grad, alpha, Li = eng.eval(want_grad=True)
    assert np.isfinite(cost) and np.all(np.isfinite(grad)) and np.all(np.triu(Li, 1) == 0)
    gmax = np.abs(grad).max()
    assert np.abs(grad[-J:]).max() < 1e-3 * gmax                  # phases carry no gradient
    p2 = params.copy(); p2[-J:] += np.linspace(0.0, 3.0, J)
    eng.set_params(p2)
    c2, _, _, _ = eng.eval(want_grad=False)
    assert abs(float(c2) - float(cost)) < 1e-5 * max(1.0, abs(float(cost)))
    # forward-only == forward of the gradient call; evaluation is deterministic
    eng.set_params(params)
    c3, _, a3, _ = eng.eval(want_grad=False)
    c4, g4, _, _ = eng.eval(want_grad=True)
    assert float(c3) == float(cost) and np.array_equal(a3, alpha) and np.array_equal(g4, grad)
    # Li really inverts the Cholesky factor of G + lam I  (checked through alpha = B g)
    eng.pass1()
    Kp = eng.dims()['Kp']
    x1 = eng.debug_read('G', (Kp * Kp + Kp,))
    G = x1[:Kp * Kp].reshape(Kp, Kp)[:K, :K]; g = x1[Kp * Kp:Kp * Kp + K]
    s2 = np.exp(2 * params[1]) * 2.0 / M
    assert np.allclose(np.diag(G)[:J] + np.diag(G)[J:], N * s2, rtol=2e-6)
    A = G + (np.exp(2 * params[0]) + 1e-6) * np.eye(K)
    assert rel(A @ alpha.ravel(), g) < 1e-7
    eng.close()
    # the fp64 mode (oracle-exact at every size the oracle can reach) on the SAME 1e6 rows:
    # fp32 mode must stay within its stated tolerances of it at full size
    e64 = HipEngine(D, S, M, dtype='f64')
    e64.set_params(params); e64.set_data(X, y)
    c64, g64, a64, L64 = e64.eval(want_grad=True)
    e64.close()
    # measured at this size (bench.py `parity_at_size`, round 2): cost 2e-11...7e-11, gradient blocks (a,b,c) 3e-11...1e-10,
    # l_F 2.8e-6, r_F 2.3e-6, alpha 4.0e-7, Li 4.5e-8; the bounds are about ten times that
    measured = dict(cost=abs(float(cost) - float(c64)) / abs(float(c64)), alpha=rel(alpha, a64), Li=rel(Li, L64))
    for nm, u, v in zip(('grad_abc', 'grad_lF', 'grad_rF'), grad_blocks(grad, D, S, M), grad_blocks(g64, D, S, M)):
        measured[nm] = rel(u, v)
    bounds = dict(cost=7e-10, grad_abc=1e-9, grad_lF=3e-5, grad_rF=3e-5, alpha=4e-6, Li=5e-7)
    print('\nheadline fp32 vs fp64: ' + ' '.join('%s %.2e' % kv for kv in measured.items()))
    for nm, bound in bounds.items():
        assert measured[nm] < bound, (nm, measured[nm], bound)


@pytest.mark.parametrize('cfg', ['C3', 'C4', 'C5'])
def test_baseline_configs_at_full_size(cfg):
    """BASELINE.json configs 3-5 at their FULL sizes (N = 1e6 / 4e6 / 1e6 rows, fp32 mode; C4's Phi has 8.7e9 elements,
    past 2^32).  The oracle cannot run there, so: size-independent properties, plus sampled entries of the Gram, of
    Phi^T y and sampled rows of the per-row adjoint scalars against float64 numpy on the same inputs."""
    import bench
    from scfgp_amd.engine import HipEngine
    N, D, S, M, dtype = bench.CONFIGS[cfg][:5]
    J = S + M; K = 2 * J
    seed = 0x5CF60030 + int(cfg[1])
    X, params = _synthetic(N, D, S, M, seed)
    eng = HipEngine(D, S, M, dtype=dtype)
    y = _teacher_targets(eng, X, D, S, M, seed)
    eng.set_params(params); eng.set_data(X, y)
    cost, grad, alpha, Li = eng.eval(want_grad=True)
    assert np.isfinite(cost) and np.all(np.isfinite(grad)) and np.all(np.triu(Li, 1) == 0)
    assert np.abs(grad[-J:]).max() < 1e-3 * np.abs(grad).max()              # phases carry no gradient
    c2, g2, a2, _ = eng.eval(want_grad=True)                                  # deterministic
    assert float(c2) == float(cost) and np.array_equal(g2, grad) and np.array_equal(a2, alpha)
    p2 = params.copy(); p2[-J:] += np.linspace(0.0, 3.0, J)                   # phase-shift invariance of the cost
    eng.set_params(p2)
    c3 = eng.eval(want_grad=False)[0]
    assert abs(float(c3) - float(cost)) < 1e-5 * max(1.0, abs(float(cost)))
    eng.set_params(params)
    # sampled Gram entries / Phi^T y over ALL rows: the phases of a few columns in float64 numpy
    a_, b_, c_, l_F, r_F, F, l_FC, FC = O.unpack_params(params, D, S, M)
    cols = np.array([0, 1, S, J // 2, J - 1])                                 # indices into the J phases
    W = np.concatenate([l_F, F], 1)[:, cols]; off = np.concatenate([l_FC, FC], 1)[:, cols]
    Zc = X @ W + off                                                          # (N, 5)
    s = np.exp(b_) * np.sqrt(2.0 / M)
    Pc, Ps = s * np.cos(Zc), s * np.sin(Zc)                                   # Phi columns cols and J + cols
    eng.pass1()
    Kp = eng.dims()['Kp']
    x1 = eng.debug_read('G', (Kp * Kp + Kp,))
    G = x1[:Kp * Kp].reshape(Kp, Kp); g = x1[Kp * Kp:Kp * Kp + K]
    idx = np.concatenate([cols, J + cols])
    Pall = np.concatenate([Pc, Ps], 1)
    assert rel(G[np.ix_(idx, idx)], Pall.T @ Pall) < 2e-6
    assert rel(g[idx], Pall.T @ y.ravel()) < 2e-5
    assert np.allclose(np.diag(G)[:J] + np.diag(G)[J:K], N * s * s, rtol=2e-6)      # cos^2 + sin^2
    A = G[:K, :K] + (np.exp(2 * a_) + 1e-6) * np.eye(K)
    assert rel(A @ alpha.ravel(), g) < 1e-6                                   # alpha solves the normal equations
    # sampled rows of p_n = 2 (mu_n - y_n) / d_n, incl. the very last rows (row offsets past 2^32 elements at C4)
    eng.factor(); eng.pass2(True)
    rows = np.unique(np.concatenate([np.arange(3), np.random.default_rng(1).integers(0, N, 20), np.arange(N - 3, N)]))
    pn = eng.debug_read('p', (eng.dims()['Np'],))[rows]
    B = eng.debug_read('B', (Kp, Kp))[:K, :K]
    Phi_r = O.feature_map(X[rows], params, D, S, M)
    mu = Phi_r @ alpha.ravel(); v = np.einsum('nk,kl,nl->n', Phi_r, B, Phi_r)
    d = np.log1p(np.exp(c_)) * (v + 1.0)
    assert rel(pn, 2.0 * (mu - y.ravel()[rows]) / d) < 1e-3, rel(pn, 2.0 * (mu - y.ravel()[rows]) / d)
    eng.close()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [2, 4, 8])
def test_row_shards_on_one_gpu_equal_single(R):
    """Row sharding through the staged C ABI: R contexts (the rank counts of BASELINE config 4), each with its block
    of the rows, their exchange buffers summed as torch tensors aliasing the library's device memory."""
    import torch
    from scfgp_amd.engine import HipEngine
    from scfgp_amd.sharded import shard_rows
    name = 'c2_small_n'
    N, D, S, M, T, seed = CASES[name]
    X, y, params, _ = case_inputs(name)
    single = HipEngine(D, S, M); single.set_params(params); single.set_data(X, y)
    c0, g0, a0, L0 = single.eval(want_grad=True)
    stream = torch.cuda.current_stream().cuda_stream
    engs = []
    for r in range(R):
        lo, hi = shard_rows(N, r, R)
        e = HipEngine(D, S, M, stream=stream)
        e.set_params(params); e.set_data(np.ascontiguousarray(X[lo:hi]), np.ascontiguousarray(y[lo:hi]), n_global=N)
        engs.append(e)

    def allsum(stage):
        bufs = [e.exchange(stage) for e in engs]
        tot = bufs[0].clone()
        for b in bufs[1:]:
            tot += b
        for b in bufs:
            b.copy_(tot)

    for want_grad in (True, False):
        for e in engs: e.pass1()
        allsum(1)
        for e in engs: e.factor()
        for e in engs: e.pass2(want_grad)
        allsum(2)
        if want_grad:
            for e in engs: e.adjoint()
            for e in engs: e.pass3()
            allsum(3)
        outs = [e.finish(want_grad) for e in engs]
        for c, g, a, L in outs:
            assert abs(float(c) - float(c0)) < 1e-12 * abs(float(c0))
            assert rel(a, a0) < 1e-10 and rel(L, L0) < 1e-11
            if want_grad:
                assert rel(g, g0) < 1e-10
    for e in engs + [single]:
        e.close()


def test_facade_fit_predict_save_load(tmp_path):
    """SCFGP.set_data / optimize / predict / save / load end to end on a small synthetic set."""
    from scfgp_amd import SCFGP
    rng = np.random.default_rng(5)
    np.random.seed(5)
    X = rng.uniform(-2, 2, (300, 3))
    y = (np.sin(X[:, :1]) + 0.5 * X[:, 1:2] ** 2 + 0.05 * rng.standard_normal((300, 1)))
    model = SCFGP(sparsity=3, nfeats=12)
    model.set_data(X[:240], y[:240])
    model.optimize(X[240:], y[240:], max_iter=40,
                   algo={'algo': 'adam', 'algo_params': {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}})
    costs = model.evals['COST'][1]
    assert len(costs) >= 30 and costs[-1] < costs[0]
    assert len(model.evals['MSE'][1]) == len(costs)
    mu, sd = model.predict(X[240:])
    assert mu.shape == (60, 1) and sd.shape == (60, 1) and np.all(sd > 0)
    assert model.evals['NMSE'][1][-1] < 0.5
    model.predict(X[240:], y[240:])
    host_metrics = {k: model.evals[k][1][-1] for k in ('MAE', 'NMAE', 'MSE', 'NMSE', 'MNLP', 'SCORE')}
    model.device_scaler = True                                # same prediction, scalers and metrics on the GPU
    mu_d, sd_d = model.predict(X[240:], y[240:])
    assert np.allclose(mu_d, mu, rtol=1e-9) and np.allclose(sd_d, sd, rtol=1e-9)
    for k, v in host_metrics.items():
        assert abs(model.evals[k][1][-1] - v) <= 1e-9 * max(1.0, abs(v)), k
    model.device_scaler = False
    path = os.path.join(str(tmp_path), 'm.npz')
    model.save(path)
    m2 = SCFGP(sparsity=1, nfeats=1); m2.load(path)
    mu2, sd2 = m2.predict(X[240:])
    assert np.allclose(mu2, mu, rtol=1e-10) and np.allclose(sd2, sd, rtol=1e-10)
    # a triple handed to another model keeps training ITS vector
    m3 = SCFGP(sparsity=3, nfeats=12); m3.set_data(X[:240], y[:240])
    before = model.params.get_value()
    m3.optimize(None, None, model.get_compiled_funcs(), max_iter=3)
    assert not np.array_equal(model.params.get_value(), before)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('algo,kw', [('adam', {'learning_rate': 0.02, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}),
                                      ('adamax', {'learning_rate': 0.02}), ('sgd', {'learning_rate': 1e-3}),
                                      ('adagrad', {'learning_rate': 0.05}), ('adadelta', {'learning_rate': 1.0}),
                                      ('rmsprop', {'learning_rate': 0.01, 'rho': 0.9, 'epsilon': 1e-6})])
def test_device_optimizer_matches_host_rules(algo, kw):
    """n iterations with the update rule on the device (one hipGraph launch per iteration) follow the
    host-side rule (the reference's Optimizer arithmetic incl. its Nesterov placement) step for step."""
    from scfgp_amd.funcs import CompiledFuncs
    name = 'c1_boston_shape'
    N, D, S, M, T, seed = CASES[name]
    X, y, params, _ = case_inputs(name)
    host = CompiledFuncs(D, S, M, params.copy(), algo, kw)
    dev = CompiledFuncs(D, S, M, params.copy(), algo, kw, device_optimizer=True)
    n = 7
    costs_h = [float(host.train_iter_func(X, y)[0]) for _ in range(n)]
    hist, alpha, Li = dev.train_iters(X, y, n)
    assert np.allclose(hist, costs_h, rtol=1e-9, atol=0)
    assert rel(dev.params.get_value(), host.params.get_value()) < 1e-6      # adamax divides by max(|g|) of near-zero entries
    # alpha / Li belong to the LAST evaluation (pre-update parameters of iteration n)
    c_more = dev.train_iter_func(X, y)                       # single-step path in device mode
    c_h = host.train_iter_func(X, y)
    assert abs(float(c_more[0]) - float(c_h[0])) < 1e-9 * abs(float(c_h[0]))
    assert rel(c_more[1], c_h[1]) < 1e-5 and rel(c_more[2], c_h[2]) < 1e-5     # fma contraction in the device rule x cond(A)
    # graph replay == eager launches
    eager = CompiledFuncs(D, S, M, params.copy(), algo, kw, device_optimizer=True)
    eager.engine.set_option('use_graph', 0)
    hist_e, _, _ = eager.train_iters(X, y, n)
    assert np.array_equal(hist_e, hist)


@pytest.mark.parametrize('wrapper', ['nesterov', 'plain'])
@pytest.mark.parametrize('rule', ['sgd', 'adagrad', 'rmsprop', 'adadelta', 'adam', 'adamax'])
def test_device_update_rule_follows_the_known_answer_vectors(rule, wrapper):
    """opt_update_kernel against tests/golden/optimizer_kats.npz (literal recurrences of SCFGP/Optimizer.py, generated by
    tests/golden/make_optimizer_kats.py -- NOT against scfgp_amd/optimizer.py): the fixed gradient sequence goes in through
    scfgp_opt_step, the parameter vector, both state vectors and the Nesterov velocity come back after every step."""
    from scfgp_amd.engine import HipEngine
    z = np.load(os.path.join(GOLD, 'optimizer_kats.npz'))
    lr, r1, b2, eps = [float(v) for v in z[rule + '/kwargs']]
    D, S, M = 1, 1, 1                                            # P = 3 + 1 + 1 + 1 + 1 = 7 = the vectors' length
    eng = HipEngine(D, S, M, 'f64')
    assert eng.P == z['theta0'].size
    eng.set_params(z['theta0'])
    eng.opt_init(rule, learning_rate=lr, beta1=r1, beta2=b2, epsilon=eps, momentum=float(z['momentum']) if wrapper == 'nesterov' else -1.0)
    pre = '%s/%s/' % (rule, wrapper)
    for t, g in enumerate(z['grads']):
        theta = eng.opt_step(g)
        assert np.allclose(theta, z[pre + 'theta'][t + 1], rtol=1e-13, atol=0), (rule, wrapper, t)
        assert np.array_equal(theta, eng.get_params())
        if rule != 'sgd':
            assert np.allclose(eng.opt_state(0), z[pre + 's1'][t + 1], rtol=1e-13, atol=0)
            assert np.allclose(eng.opt_state(1), z[pre + 's2'][t + 1], rtol=1e-13, atol=0)
        if wrapper == 'nesterov':
            assert np.allclose(eng.opt_state(2), z[pre + 'vel'][t + 1], rtol=1e-13, atol=1e-300)
        assert eng.opt_state(3)[0] == t + 1
    eng.close()


def test_index_list_minibatches_on_resident_rows():
    """scfgp_eval_rows: a batch gathered on the device equals the same rows uploaded from the host, and
    the full set is back for the next plain evaluation; the facade's minibatch loop uses it."""
    from scfgp_amd.engine import HipEngine
    from scfgp_amd import SCFGP
    name = 'kin8nm_like'
    N, D, S, M, T, seed = CASES[name]
    X, y, params, _ = case_inputs(name)
    eng = HipEngine(D, S, M); eng.set_params(params); eng.set_data(X, y)
    c_full, g_full, _, _ = eng.eval(want_grad=True)
    rng = np.random.default_rng(3)
    for n in (150, 1, 999, 300):
        idx = rng.choice(N, n, replace=False)
        c, g, a, L = eng.eval_rows(idx, True)
        c0, g0, a0, L0 = O.value_and_grad(X[idx], y[idx], params, S, M)
        assert abs(float(c) - c0) < 1e-10 * abs(c0) and rel(g, g0) < 1e-7 and rel(a, a0) < 1e-7
        PB.oracle_check((c, g, a, L), X[idx], y[idx], params, S, M, 'f64', label='index list')
    c2, g2, _, _ = eng.eval(want_grad=True)                 # all rows again
    assert float(c2) == float(c_full) and np.array_equal(g2, g_full)
    with pytest.raises(ValueError):
        eng.eval_rows(np.array([0, N]), True)
    eng.close()
    np.random.seed(11)
    model = SCFGP(sparsity=4, nfeats=10)
    model.set_data(X * 3 - 1, np.sin(X[:, :1] * 5) + 0.1 * y)
    model.optimize(None, None, max_iter=6, nbatches=3, batchsize=120)
    assert len(model.evals['COST'][1]) == 7 and np.all(np.isfinite(model.evals['COST'][1]))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,D,S,M,dtype', [(3000, 8, 32, 1024, 'f32'),      # C3 shape (K = 2112), reduced N
                                           (2500, 64, 32, 1024, 'f64'),     # C4 / headline shape
                                           (1500, 512, 64, 2048, 'f32')])   # C5 shape (K = 4224)
def test_baseline_config_shapes_against_oracle(N, D, S, M, dtype):
    """The K, D, S, M of BASELINE.json's large configs at an N the CPU oracle finishes in seconds."""
    from scfgp_amd.engine import HipEngine
    seed = 0x5CF60300 + D
    X = synth.make_X(seed, N, D)
    params = synth.make_params(seed + 0x0202, D, S, M, abc=(-1.0, 0.0, -1.0))
    eng = HipEngine(D, S, M, dtype=dtype)
    y = _teacher_targets(eng, X, D, S, M, seed)
    eng.set_params(params); eng.set_data(X, y)
    cost, grad, alpha, Li = eng.eval(want_grad=True)
    c0, g0, a0, L0 = O.value_and_grad(X, y, params, S, M, chunk=1024)
    if dtype == 'f64':
        assert abs(float(cost) - c0) < 1e-10 * abs(c0) and rel(grad, g0) < 1e-8 and rel(alpha, a0) < 1e-7 and rel(Li, L0) < 1e-8
    else:
        assert abs(float(cost) - c0) < 1e-5 * max(1.0, abs(c0))
        for u, v in zip(grad_blocks(grad, D, S, M), grad_blocks(g0, D, S, M)):
            assert rel(u, v) < 1e-3
        assert rel(Li, L0) < 1e-3
    PB.oracle_check((cost, grad, alpha, Li), X, y, params, S, M, dtype, label='baseline shape')
    eng.close()


def test_predict_in_chunks_and_call_order_errors():
    """T larger than the library's internal predict chunk; staged calls out of order are refused."""
    from scfgp_amd.engine import HipEngine
    name = 'kin8nm_like'
    N, D, S, M, T, seed = CASES[name]
    X, y, params, _ = case_inputs(name)
    eng = HipEngine(D, S, M); eng.set_params(params); eng.set_data(X, y)
    c, g, alpha, Li = eng.eval(want_grad=True)
    Tbig = 70001
    Xs = synth.make_X(seed + 99, Tbig, D)
    mu, sd = eng.predict(Xs, alpha, Li)
    sel = np.r_[0:50, 32760:32780, Tbig - 50:Tbig]
    mu0, sd0 = O.predict(Xs[sel], alpha, Li, params, S, M)
    assert rel(mu[sel], mu0) < 1e-9 and rel(sd[sel], sd0) < 1e-10
    # training data survived the predict call
    c2, g2, _, _ = eng.eval(want_grad=True)
    assert float(c2) == float(c) and np.array_equal(g2, g)
    for bad in (eng.factor, eng.adjoint, eng.pass3, lambda: eng.pass2(True), lambda: eng.finish(True)):
        with pytest.raises(ValueError):
            bad()
    eng.pass1(); eng.factor(); eng.pass2(False)
    with pytest.raises(ValueError):
        eng.adjoint()                                   # forward-only pass 2 cannot feed the adjoint
    c3, _, _, _ = eng.finish(False)
    assert abs(float(c3) - float(c)) < 1e-13 * abs(float(c))
    eng.close()


@pytest.mark.parametrize('algo', ['min-max', 'normal', 'inv-normal', 'auto-normal', 'auto-inv-normal'])
def test_predict_raw_applies_the_x_scaler_on_the_device(algo):
    """scfgp_predict_raw == pred_func(X_scaler.forward_transform(Xs)) for every scaler mode (SCFGP.py:279)."""
    from scfgp_amd.engine import HipEngine
    from scfgp_amd.scaler import Scaler
    rng = np.random.default_rng(12)
    Xraw = np.exp(rng.standard_normal((400, 6))); Xraw[:, 3] = 2.5                  # one constant column is dropped
    sc = Scaler(algo); sc.fit(Xraw)
    D, S, M = 5, 3, 8
    params = O.init_params(D, S, M, rng); params[:3] = (-0.5, 0.0, -0.8)
    Xt = np.ascontiguousarray(sc.forward_transform(Xraw)); y = rng.standard_normal((400, 1))
    eng = HipEngine(D, S, M); eng.set_params(params); eng.set_data(Xt, y)
    c, g, alpha, Li = eng.eval(want_grad=True)
    Xs_raw = np.exp(rng.standard_normal((333, 6))); Xs_raw[:, 3] = 2.5
    eng.set_x_scaler(sc)
    mu_r, sd_r = eng.predict_raw(Xs_raw, alpha, Li)
    mu_h, sd_h = eng.predict(np.ascontiguousarray(sc.forward_transform(Xs_raw)), alpha, Li)
    assert rel(mu_r, mu_h) < 1e-11 and rel(sd_r, sd_h) < 1e-11
    eng.close()


@pytest.mark.parametrize('xalgo,yalgo,T', [('auto-inv-normal', 'auto-normal', 333), ('min-max', 'min-max', 500),
                                           ('normal', 'normal', 40000), ('inv-normal', 'inv-normal', 257),
                                           ('auto-normal', 'auto-inv-normal', 1000)])
def test_predict_y_back_transform_and_metrics_on_the_device(xalgo, yalgo, T):
    """scfgp_predict_y == the host tail of SCFGP.predict (SCFGP.py:281-293): y_scaler.backward_transform of mu and of the
    mu +- std band, std_y, and the six metrics -- for every scaler mode, one and several predict chunks."""
    from scfgp_amd.engine import HipEngine
    from scfgp_amd.scaler import Scaler
    rng = np.random.default_rng(21)
    n, D, S, M = 400, 4, 3, 10
    Xraw = np.exp(0.5 * rng.standard_normal((n, D)))
    yraw = np.exp(0.3 * np.sin(Xraw[:, :1]) + 0.1 * rng.standard_normal((n, 1)))
    xs, ys_ = Scaler(xalgo), Scaler(yalgo)
    xs.fit(Xraw); ys_.fit(yraw)
    Xt = np.ascontiguousarray(xs.forward_transform(Xraw)); yt = np.ascontiguousarray(ys_.forward_transform(yraw))
    params = O.init_params(D, S, M, rng); params[:3] = (-1.0, 0.0, -1.5)
    eng = HipEngine(D, S, M); eng.set_params(params); eng.set_data(Xt, yt)
    _, _, alpha, Li = eng.eval(want_grad=True)
    Xs_raw = np.exp(0.5 * rng.standard_normal((T, D)))
    ys_raw = np.exp(0.3 * np.sin(Xs_raw[:, :1]) + 0.1 * rng.standard_normal((T, 1)))
    eng.set_x_scaler(xs); eng.set_y_scaler(ys_)
    mu_y, sd_y, met = eng.predict_y(Xs_raw, alpha, Li, ys_raw)
    # host tail, as model.predict writes it
    mu_f, sd_f = eng.predict(np.ascontiguousarray(xs.forward_transform(Xs_raw)), alpha, Li)
    with np.errstate(all='ignore'):
        mu_h = ys_.backward_transform(mu_f)
        sd_h = 0.5 * (ys_.backward_transform(mu_f + sd_f[:, None]) - ys_.backward_transform(mu_f - sd_f[:, None]))
        err = mu_h - ys_raw
        mae, mse = np.mean(np.abs(err)), np.mean(err ** 2.)
        mnlp = 0.5 * np.mean((err / sd_h) ** 2 + np.log(2 * np.pi * sd_h ** 2))
        nmse = mse / np.var(ys_raw)
        ref = dict(MAE=mae, NMAE=mae / np.std(ys_raw), MSE=mse, NMSE=nmse, MNLP=mnlp, SCORE=nmse / (1 + np.exp(-mnlp)))
    assert mu_y.shape == (T, 1) and sd_y.shape == (T, 1)
    assert np.array_equal(np.isnan(mu_y), np.isnan(mu_h)) and np.array_equal(np.isnan(sd_y), np.isnan(sd_h))
    ok = ~(np.isnan(mu_h) | np.isnan(sd_h))
    # inv-normal targets: mu +- std outside (0, 1) is NaN on both sides.  The rows that stay are those the host tail keeps when it is
    # fed the CPU oracle's mu_f, std_f on these seeds (no band edge within 3e-5 of 0 or 1, so the device's last bits cannot move one)
    kept = {('auto-inv-normal', 'auto-normal', 333): 333, ('min-max', 'min-max', 500): 500, ('normal', 'normal', 40000): 40000,
            ('inv-normal', 'inv-normal', 257): 134, ('auto-normal', 'auto-inv-normal', 1000): 313}
    assert ok.sum() >= kept[(xalgo, yalgo, T)], (int(ok.sum()), xalgo, yalgo, T)
    assert np.allclose(mu_y[ok], mu_h[ok], rtol=1e-9, atol=1e-12) and np.allclose(sd_y[ok], sd_h[ok], rtol=1e-8, atol=1e-12)
    for k in ref:
        assert (np.isnan(ref[k]) and np.isnan(met[k])) or abs(met[k] - ref[k]) <= 1e-8 * max(1.0, abs(ref[k])), (k, met[k], ref[k])
    # without targets: same moments, no metrics
    mu2, sd2, met2 = eng.predict_y(Xs_raw, alpha, Li)
    assert met2 is None and np.array_equal(mu2, mu_y, equal_nan=True) and np.array_equal(sd2, sd_y, equal_nan=True)
    eng.close()
