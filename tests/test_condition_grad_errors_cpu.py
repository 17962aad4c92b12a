"""Argument checks of scfgp_condition_grad that stand before "parameters not set", in source order, on a context that needs no GPU
(tests/test_api_errors_cpu.py's pattern: without a GPU scfgp_create returns -2 and still hands back the context, with its geometry and
nothing else).  Every case asserts the status and the whole text of scfgp_last_error; a case that breaks two rules at once pins which
refusal comes first.  The checks behind "parameters not set" -- the scan of rho -- are in tests/test_gpu_condition_grad.py."""
import ctypes as C

import numpy as np
import pytest

from scfgp_amd import _lib
from scfgp_amd._lib import dptr

D, S, M = 4, 2, 3
K = 2 * (S + M)
EARG = -1

X = np.zeros((1, D)); G = np.zeros((1, D)); RHO = np.full((1, D), -1.0); Y = np.zeros(1); A = np.zeros(K); L = np.eye(K)
AO = np.full(K, 7.0); LO = np.full((K, K), 7.0)
x, g, rho, y, a, l, ao, lo = (dptr(v) for v in (X, G, RHO, Y, A, L, AO, LO))
N_ = None
_KEEP = []                                    # the arrays behind the pointers of _dims


def _dims(*v):
    _KEEP.append(np.array(v, dtype=np.int32))
    return _KEEP[-1].ctypes.data_as(C.POINTER(C.c_int32))


# condition_grad(Xn, n, dims, nd, Gn, rho, yn, alpha, Li, mode, alpha_out, Li_out); the status is SCFGP_EARG throughout
CASES = [
    ((N_, 1, N_, D, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: bad arguments'),
    ((x, 1, N_, D, N_, N_, N_, a, l, 0, ao, lo), 'condition_grad: bad arguments'),
    ((x, 1, N_, D, g, N_, N_, N_, l, 0, ao, lo), 'condition_grad: bad arguments'),
    ((x, 1, N_, D, g, N_, N_, a, N_, 0, ao, lo), 'condition_grad: bad arguments'),
    ((x, 1, N_, D, g, N_, N_, a, l, 0, N_, lo), 'condition_grad: bad arguments'),
    ((x, 1, N_, D, g, N_, N_, a, l, 0, ao, N_), 'condition_grad: bad arguments'),
    ((x, 0, N_, D, N_, N_, N_, a, l, 0, ao, lo), 'condition_grad: bad arguments'),                     # a NULL Gn and n = 0
    ((x, 0, N_, D, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: n must be at least 1'),
    ((x, -2, N_, 0, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: n must be at least 1'),                # n < 1 and nd = 0
    ((x, 1, N_, 0, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: nd must lie in 1..D'),
    ((x, 1, N_, D + 1, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: nd must lie in 1..D'),
    ((x, 1, _dims(0, 0, 0, 0, 0), D + 1, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: nd must lie in 1..D'),       # and repeated entries
    ((x, 1, N_, D - 1, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: dims == NULL needs nd == D'),
    ((x, 1, N_, 1, g, N_, N_, a, l, 3, ao, lo), 'condition_grad: dims == NULL needs nd == D'),            # and a bad mode
    ((x, 1, _dims(0, D), 2, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: dims[1] is out of range or repeated'),
    ((x, 1, _dims(-1, 2), 2, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: dims[0] is out of range or repeated'),
    ((x, 1, _dims(3, 1, 3), 3, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: dims[2] is out of range or repeated'),
    ((x, 1, _dims(3, 1, 1, 9), 4, g, N_, N_, a, l, 0, ao, lo), 'condition_grad: dims[2] is out of range or repeated'),   # the first bad entry
    ((x, 1, _dims(1, 1), 2, g, N_, N_, a, l, 2, ao, lo), 'condition_grad: dims[1] is out of range or repeated'),   # and a bad mode
    ((x, 1, N_, D, g, N_, N_, a, l, 2, ao, lo), 'condition_grad: bad mode'),
    ((x, 1, N_, D, g, N_, N_, a, l, -1, ao, lo), 'condition_grad: bad mode'),
    ((x, 1, _dims(2, 0), 2, g, N_, y, a, l, 1, ao, lo), 'condition_grad: no X scaler set'),
    ((x, 1, N_, D, g, rho, N_, a, l, 1, ao, lo), 'condition_grad: no X scaler set'),                    # and a negative rho
    ((x, 1, N_, D, g, rho, N_, a, l, 0, ao, lo), 'condition_grad: parameters not set'),                 # rho is not read before the model
    ((x, 1, _dims(3, 0, 2, 1), D, g, N_, y, a, l, 0, ao, lo), 'condition_grad: parameters not set'),
]


@pytest.fixture(scope='module')
def ctx():
    lib = _lib.load()
    c = C.c_void_p()
    rc = lib.scfgp_create(C.byref(c), D, S, M, 0, 0, None)
    assert rc in (0, -2) and c.value            # -2 without a GPU: the context is there all the same
    yield lib, c
    lib.scfgp_destroy(c)


@pytest.mark.parametrize('case', range(len(CASES)))
def test_refusal(ctx, case):
    lib, c = ctx
    args, text = CASES[case]
    assert lib.scfgp_condition_grad(c, *args) == EARG
    assert lib.scfgp_last_error(c).decode() == text
    assert np.all(AO == 7.0) and np.all(LO == 7.0)


def test_null_context():
    assert _lib.load().scfgp_condition_grad(None, *CASES[-1][0]) == EARG


def test_a_point_may_not_bring_more_rows_than_a_chunk_holds():
    """nb > 32768 needs D >= 32768: a context of that width, which no GPU has to back (J = 2 keeps its geometry small)"""
    lib = _lib.load()
    c = C.c_void_p()
    Dw = 32768
    rc = lib.scfgp_create(C.byref(c), Dw, 1, 1, 0, 0, None)
    assert rc in (0, -2) and c.value
    try:
        Xw = np.zeros((1, Dw)); Gw = np.zeros((1, Dw)); Kw = 4
        args = lambda yy: (dptr(Xw), 1, None, Dw, dptr(Gw), None, yy, dptr(np.zeros(Kw)), dptr(np.eye(Kw)), 0, dptr(np.zeros(Kw)), dptr(np.zeros((Kw, Kw))))
        assert lib.scfgp_condition_grad(c, *args(dptr(np.zeros(1)))) == EARG
        assert lib.scfgp_last_error(c).decode() == 'condition_grad: the rows of a point (nd, and one for its value) must not exceed 32768'
        assert lib.scfgp_condition_grad(c, *args(None)) == EARG          # nb = 32768 is allowed: the next refusal
        assert lib.scfgp_last_error(c).decode() == 'condition_grad: parameters not set'
    finally:
        lib.scfgp_destroy(c)
