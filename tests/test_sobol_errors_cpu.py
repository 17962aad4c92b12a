"""The declaration, the binding and the argument checks of scfgp_sobol that stand before "parameters not set", in source order, on a
context that needs no GPU (tests/test_api_errors_cpu.py's pattern: without a GPU scfgp_create returns -2 and still hands back the
context, with its geometry and nothing else).  Every case asserts the status, the whole text of scfgp_last_error and that the outputs
kept their sentinel; a case that breaks two rules at once pins which refusal comes first.  The checks behind "parameters not set" --
the finite scans of the measure and of W -- are in tests/test_gpu_sobol.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scfgp_amd import _lib
from scfgp_amd._lib import dptr

D, S, M = 4, 2, 3
K = 2 * (S + M)
EARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P0 = np.zeros(D); P1 = np.ones(D); PNEG = np.array([1.0, 1.0, -1.0, 1.0]); PNAN = np.array([0.0, np.nan, 0.0, 0.0])
W = np.full((K, 2), np.nan)                   # never read before the model: a finite scan comes behind "parameters not set"
F0 = np.full(2, 7.0); V = np.full(2, 7.0); VM = np.full((2, D), 7.0); VT = np.full((2, D), 7.0); PB = np.full(K, 7.0)
OUTS = (F0, V, VM, VT, PB)
p0, p1, pneg, pnan, w, f0, v, vm, vt, pb = (dptr(a) for a in (P0, P1, PNEG, PNAN, W, F0, V, VM, VT, PB))
N_ = None
_KEEP = []


def _kind(*k):
    _KEEP.append(np.array(k, dtype=np.int32))
    return _KEEP[-1].ctypes.data_as(C.POINTER(C.c_int32))


# sobol(kind, p0, p1, W, nw, f0, V, Vmain, Vtot, phibar); the status is SCFGP_EARG throughout
CASES = [
    ((N_, N_, p1, w, 2, f0, v, vm, vt, pb), 'sobol: p0 and p1 are needed'),
    ((N_, p0, N_, w, 2, f0, v, vm, vt, pb), 'sobol: p0 and p1 are needed'),
    ((N_, N_, p1, w, 2, N_, N_, N_, N_, N_), 'sobol: p0 and p1 are needed'),                       # and no output
    ((N_, p0, p1, w, 2, N_, N_, N_, N_, N_), 'sobol: no output asked for'),
    ((N_, p0, p1, N_, 0, N_, N_, N_, N_, N_), 'sobol: no output asked for'),                       # and no W, nw = 0
    ((N_, p0, p1, N_, 2, f0, N_, N_, N_, N_), 'sobol: W is needed for f0, V, Vmain and Vtot'),
    ((N_, p0, p1, N_, 2, N_, v, N_, N_, pb), 'sobol: W is needed for f0, V, Vmain and Vtot'),
    ((N_, p0, p1, N_, 2, N_, N_, vm, N_, N_), 'sobol: W is needed for f0, V, Vmain and Vtot'),
    ((N_, p0, p1, N_, 0, N_, N_, N_, vt, N_), 'sobol: W is needed for f0, V, Vmain and Vtot'),      # and nw = 0
    ((N_, p0, p1, w, 0, f0, v, vm, vt, pb), 'sobol: nw must lie in 1..1024'),
    ((N_, p0, p1, w, -3, N_, v, N_, N_, N_), 'sobol: nw must lie in 1..1024'),
    ((N_, p0, p1, w, 1025, N_, N_, N_, vt, N_), 'sobol: nw must lie in 1..1024'),
    ((_kind(0, 1, 2, 0), p0, p1, w, 1025, f0, N_, N_, N_, N_), 'sobol: nw must lie in 1..1024'),      # and a bad kind
    ((_kind(0, 1, 2, 0), p0, p1, w, 2, f0, v, vm, vt, pb), 'sobol: kind[2] must be 0 (uniform) or 1 (normal)'),
    ((_kind(-1, 1, 2, 0), p0, p1, N_, 0, N_, N_, N_, N_, pb), 'sobol: kind[0] must be 0 (uniform) or 1 (normal)'),   # phibar alone: nw is not read
    ((_kind(0, 0, 0, 7), p0, pneg, w, 2, f0, v, vm, vt, pb), 'sobol: kind[3] must be 0 (uniform) or 1 (normal)'),      # and a bad range
    ((N_, p0, pneg, w, 2, f0, v, vm, vt, pb), 'sobol: input 2: p1 < p0 on a uniform input'),
    ((_kind(0, 0, 0, 0), p1, p0, w, 2, f0, v, vm, vt, pb), 'sobol: input 0: p1 < p0 on a uniform input'),             # the first of four
    ((_kind(0, 0, 1, 0), p0, pneg, w, 2, f0, v, vm, vt, pb), 'sobol: input 2: p1 (the standard deviation) is negative'),
    ((_kind(1, 1, 1, 1), p1, p0, w, 2, f0, v, vm, vt, pb), 'sobol: parameters not set'),              # normal: a zero sd below the mean is fine
    ((N_, p0, p0, w, 2, f0, v, vm, vt, pb), 'sobol: parameters not set'),                            # point masses
    ((N_, pnan, p1, w, 2, f0, v, vm, vt, pb), 'sobol: parameters not set'),                          # values are not scanned before the model
    ((N_, p0, p1, N_, 0, N_, N_, N_, N_, pb), 'sobol: parameters not set'),
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
    assert lib.scfgp_sobol(c, *args) == EARG
    assert lib.scfgp_last_error(c).decode() == text
    assert all(np.all(o == 7.0) for o in OUTS)


def test_null_context():
    assert _lib.load().scfgp_sobol(None, *CASES[-1][0]) == EARG


def test_the_option_is_known(ctx):
    lib, c = ctx
    assert lib.scfgp_set_option(c, b'test_sobol_group', 3) == 0


def test_declaration_matches_the_binding():
    """include/scfgp_hip.h declares what _lib.SIGNATURES binds: the same number of arguments, pointer for pointer"""
    text = open(os.path.join(ROOT, 'include', 'scfgp_hip.h')).read()
    m = re.search(r'^int scfgp_sobol\(([^;]*)\);', text, re.M | re.S)
    assert m, 'scfgp_sobol is not declared'
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    res, args = _lib.SIGNATURES['scfgp_sobol']
    assert res is C.c_int and len(params) == len(args) == 11
    for p, a in zip(params, args):
        if a is C.c_int:
            assert p.startswith('int ') and '*' not in p, p
        elif a is C.c_void_p:
            assert p.startswith('scfgp_ctx*'), p
        elif a._type_ is C.c_int32:
            assert p.startswith('const int32_t*'), p
        else:
            assert a._type_ is C.c_double and 'double*' in p, p
