import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ['SCFGP_LIB_VARIANT'] = '_asan'
from scfgp_amd import _lib
lib = _lib.load()
ctx = C.c_void_p()
assert lib.scfgp_create(C.byref(ctx), 0, 1, 1, 0, 0, None) == -1
assert lib.scfgp_create(None, 4, 2, 3, 0, 0, None) == -1
assert lib.scfgp_last_error(None) == b'null context'
n = 0
for (D, S, M) in [(13, 8, 64), (64, 32, 1024), (512, 64, 2048), (3, 2, 3), (8, 2, 190)]:
    for N in (1, 257, 506, 100000, 1000000, 4000000):
        for dt in (0, 1):
            for ns in (0, 1, 7, 16, 48, 1000):
                for tp in (0, 1):
                    assert lib.scfgp_selftest_row_splits(D, S, M, N, dt, ns, tp) == 0
                    n += 1
# argument errors of scfgp_predict_cov that need no device: the null context, and (where a context exists) every check that precedes
# the first device call
x = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
xp = C.cast(x, C.POINTER(C.c_double))
assert lib.scfgp_predict_cov(None, xp, 1, None, 0, xp, 0, 0, xp) == -1
n += 1
# a context on a GPU-less box: create fails cleanly inside hipSetDevice / hipMalloc, the error text is readable, destroy is safe
rc = lib.scfgp_create(C.byref(ctx), 4, 2, 3, 0, 0, None)
print('create on a GPU-less box ->', rc, lib.scfgp_last_error(ctx) if ctx else None)
if ctx:
    for args in [(None, 1, None, 0, xp, 0, 0, xp), (xp, 0, None, 0, xp, 0, 0, xp), (xp, 1, xp, 0, xp, 0, 0, xp),
                 (xp, 1, xp, 32769, xp, 0, 0, xp), (xp, 1, xp, 1, xp, 0, 1, xp), (xp, 1, None, 0, xp, 1, 0, xp),
                 (xp, 1, None, 0, xp, 2, 0, xp), (xp, 1, None, 0, xp, 0, 0, xp)]:     # the last: parameters not set
        assert lib.scfgp_predict_cov(ctx, *args) == -1 and lib.scfgp_last_error(ctx).startswith(b'predict_cov')
        n += 1
# scfgp_acquire: the same -- every argument check precedes the first device call
ip = C.cast((C.c_int64 * 1)(0), C.POINTER(C.c_int64))
assert lib.scfgp_acquire(None, xp, 1, None, xp, xp, 2, xp, 2, None, 0, 0, 0, 0, xp, ip, xp, None, None, None) == -1
n += 1
if ctx:
    for args in [(None, 1, None, xp, xp, 2, xp, 2, None, 0, 0, 0, 0, xp, ip, xp, None, None, None),      # NULL Xs
                 (xp, 0, None, xp, xp, 2, xp, 2, None, 0, 0, 0, 0, xp, ip, xp, None, None, None),        # T < 1
                 (xp, 1, None, xp, xp, 5, xp, 2, None, 0, 0, 0, 0, xp, ip, xp, None, None, None),        # kind
                 (xp, 1, None, xp, xp, 2, xp, 2, None, 0, 2, 0, 0, xp, ip, xp, None, None, None),        # mode
                 (xp, 1, None, xp, xp, 2, xp, 1, None, 0, 0, 0, 0, xp, ip, xp, None, None, None),        # npar
                 (xp, 1, None, xp, xp, 2, None, 2, None, 0, 0, 0, 0, xp, ip, xp, None, None, None),      # NULL par
                 (xp, 1, None, xp, xp, 4, None, 0, None, 3, 0, 0, 0, xp, ip, xp, None, None, None),      # MES without fstar
                 (xp, 1, None, xp, xp, 4, None, 0, xp, 1025, 0, 0, 0, xp, ip, xp, None, None, None),     # nstar
                 (xp, 1, None, xp, xp, 2, xp, 2, xp, 1, 0, 0, 0, xp, ip, xp, None, None, None),          # fstar for EI
                 (xp, 1, None, xp, xp, 2, xp, 2, None, 0, 0, 0, 0, None, None, None, xp, xp, None),      # no output
                 (xp, 1, None, xp, xp, 2, xp, 2, None, 0, 0, 0, 0, xp, None, xp, None, None, None),      # val without idx
                 (xp, 1, None, xp, xp, 2, xp, 2, None, 0, 1, 0, 0, xp, ip, xp, None, None, None),        # no X scaler
                 (xp, 1, None, xp, xp, 2, xp, 2, None, 0, 0, 0, 0, xp, ip, xp, None, None, None)]:       # parameters not set
        assert lib.scfgp_acquire(ctx, *args) == -1 and lib.scfgp_last_error(ctx).startswith(b'acquire')
        n += 1
# scfgp_acquire_kg: the same
z3 = C.cast((C.c_double * 5)(-1.0, 0.0, 1.0, 2.0, 3.0), C.POINTER(C.c_double))
assert lib.scfgp_acquire_kg(None, xp, 1, None, None, 0, xp, xp, z3, 3, 0, 1, 0, xp, xp, ip, xp, None, None) == -1
n += 1
if ctx:
    for args in [(None, 1, None, None, 0, xp, xp, z3, 3, 0, 1, 0, xp, xp, ip, xp, None, None),           # NULL Xc
                 (xp, 1, None, None, 0, xp, xp, None, 3, 0, 1, 0, xp, xp, ip, xp, None, None),           # NULL z
                 (xp, 0, None, None, 0, xp, xp, z3, 3, 0, 1, 0, xp, xp, ip, xp, None, None),             # T < 1
                 (xp, 32769, None, None, 0, xp, xp, z3, 3, 0, 1, 0, xp, xp, ip, xp, None, None),         # the symmetric form's bound
                 (xp, 1, None, xp, 0, xp, xp, z3, 3, 0, 1, 0, xp, xp, ip, xp, None, None),               # R < 1
                 (xp, 1, None, xp, 32769, xp, xp, z3, 3, 0, 1, 0, xp, xp, ip, xp, None, None),           # R
                 (xp, 1, None, None, 0, xp, xp, z3, 2, 0, 1, 0, xp, xp, ip, xp, None, None),             # J
                 (xp, 1, None, None, 0, xp, xp, z3, 33, 0, 1, 0, xp, xp, ip, xp, None, None),            # J
                 (xp, 1, None, None, 0, xp, xp, xp, 3, 0, 1, 0, xp, xp, ip, xp, None, None),             # nodes not increasing
                 (xp, 1, None, None, 0, xp, xp, C.cast(C.byref(z3.contents, 16), C.POINTER(C.c_double)), 3, 0, 1, 0, xp, xp, ip, xp, None,
                  None),                                                                                 # no 0.0 among the nodes (1, 2, 3)
                 (xp, 1, None, None, 0, xp, xp, z3, 4, 2, 1, 0, xp, xp, ip, xp, None, None),             # mode
                 (xp, 1, None, None, 0, xp, xp, z3, 3, 0, 1, 0, None, None, None, None, None, None),     # no output
                 (xp, 1, None, None, 0, xp, xp, z3, 3, 0, 1, 0, xp, xp, None, xp, None, None),           # val without idx
                 (xp, 1, None, None, 0, xp, xp, z3, 3, 1, 1, 0, xp, xp, ip, xp, None, None),             # no X scaler
                 (xp, 1, None, None, 0, xp, xp, z3, 3, 0, 1, 0, xp, xp, ip, xp, None, None)]:            # parameters not set
        assert lib.scfgp_acquire_kg(ctx, *args) == -1 and lib.scfgp_last_error(ctx).startswith(b'acquire_kg')
        n += 1
# scfgp_predict_gradcov: the same (the weights are checked on the host before the first device call too, but behind the parameters)
assert lib.scfgp_predict_gradcov(None, xp, 1, None, xp, xp, 0, xp, xp, xp, xp) == -1
n += 1
if ctx:
    for args in [(None, 1, None, xp, xp, 0, xp, xp, xp, xp),                                             # NULL Xs
                 (xp, 1, None, None, xp, 0, xp, xp, xp, xp),                                             # NULL alpha
                 (xp, 1, None, xp, None, 0, xp, xp, xp, xp),                                             # NULL Li
                 (xp, 0, None, xp, xp, 0, xp, xp, xp, xp),                                               # T < 1
                 (xp, 1, None, xp, xp, 2, xp, xp, xp, xp),                                               # mode
                 (xp, 1, xp, xp, xp, 0, None, None, None, None),                                         # no output
                 (xp, 1, None, xp, xp, 1, xp, xp, xp, xp),                                               # no X scaler
                 (xp, 1, None, xp, xp, 0, xp, None, None, xp)]:                                          # parameters not set
        assert lib.scfgp_predict_gradcov(ctx, *args) == -1 and lib.scfgp_last_error(ctx).startswith(b'predict_gradcov')
        n += 1
if ctx: lib.scfgp_destroy(ctx)
print('host-side calls under ASan/UBSan:', n + 4, 'ok')
