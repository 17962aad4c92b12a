"""
What scfgp_amd.engine.HipEngine's posterior and pool methods (predict .. select_qei, and condition() without arguments) hand to the C
ABI and hand back to their caller, recorded with a double in place of the shared library: no GPU and no libscfgp_hip.so is needed.

    python tests/golden/make_engine_calls.py        ->  tests/golden/engine_calls.json

The fixture is a record of the engine.py it was generated from; tests/test_engine_marshal.py runs the same scenarios against the
engine.py of the tree and compares.  Regenerate it only when a method's behaviour is meant to change.

  the double     HipEngine.__new__ with D, S, M = 4, 2, 3 set by hand and `lib` an object that records every call.  It returns the
                 status of the scenario; on status 0 (and on -4, whose outputs a delivering entry point has written) it fills output
                 array number p of the call with 1000 p + arange(size).  Which positions are outputs is the table OUTPUTS, read off
                 include/scfgp_hip.h.  scfgp_get_dims fills slot 7 (the resident rows) with T; scfgp_last_error returns ERROR_TEXT.
  a call         the entry point's name and per argument: a scalar's Python type and value; for a pointer NULL or the dtype, shape
                 and C-contiguity of the array behind it (numpy keeps it in ._arr), for an input also its values and the name of the
                 caller's argument whose memory it is ('of'; 'is': the very same object -- no copy was made).
  a result       the structure, keys, Python types, dtypes, shapes and values of what the method returns, or the exception's type and
                 whole text.  A refusal before the call shows as an empty list of calls.
  values         up to 8 elements as float.hex / int, more as the SHA-1 of the array's bytes (the inputs are deterministic, below).

Scenario names: ok/ the plain accepted call per method and mode, full/ with every optional input and output, cast/ with a
non-contiguous float32 row array and a list for w, bad/ one faulty argument, range/ a count outside the library's range, rc/ a status.
"""
import hashlib
import json
import os
import sys
from collections import OrderedDict
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from scfgp_amd import _lib                                     # noqa: E402
from scfgp_amd.engine import HipEngine                         # noqa: E402

PATH = os.path.join(HERE, 'engine_calls.json')
D, S, M = 4, 2, 3
T, R = 5, 3
D_RAW, XCOLS = 6, [0, 2, 3, 5]
K = 2 * (S + M)
ERROR_TEXT = 'the double refuses'
STATUSES = (-1, -2, -3, -4, -5, _lib.SCFGP_REDO)

# argument positions (ctx is 0) that the entry point writes
OUTPUTS = {
    'scfgp_predict': (5, 6), 'scfgp_predict_raw': (5, 6), 'scfgp_predict_y': (6, 7, 8), 'scfgp_predict_grad': (6, 7, 8, 9),
    'scfgp_predict_gradcov': (7, 8, 9, 10), 'scfgp_predict_pd': (11, 12, 13, 14), 'scfgp_sample_weights': (5,), 'scfgp_sample': (9,),
    'scfgp_sample_argmax': (10, 11), 'scfgp_sample_grad': (7, 8), 'scfgp_acquire': (14, 15, 16, 17, 18, 19),
    'scfgp_acquire_kg': (13, 14, 15, 16, 17, 18), 'scfgp_predict_cov': (8,), 'scfgp_condition': (7, 8), 'scfgp_forget': (7, 8, 9, 10, 11),
    'scfgp_loo': (8, 9, 10, 11), 'scfgp_select': (7, 8, 9, 10), 'scfgp_select_iv': (10, 11, 12, 13, 14),
    'scfgp_select_qei': (15, 16, 17, 18, 19), 'scfgp_get_condition': (1,),
}


def values(a):
    a = np.ascontiguousarray(a)
    if a.size <= 8:
        return [float(v).hex() if a.dtype.kind == 'f' else int(v) for v in a.reshape(-1)]
    return 'sha1:' + hashlib.sha1(a.tobytes()).hexdigest()


def describe(v):
    """what a method returned, as JSON"""
    if v is None:
        return None
    if isinstance(v, tuple):
        return {'tuple': [describe(x) for x in v]}
    if isinstance(v, dict):
        return {'dict': [[k, describe(x)] for k, x in v.items()]}
    if isinstance(v, np.ndarray):
        return {'dtype': str(v.dtype), 'shape': list(v.shape), 'values': values(v)}
    if isinstance(v, (float, np.floating)):
        return [type(v).__name__, float(v).hex()]
    return [type(v).__name__, repr(v)]


class Double(object):
    """stands in for the ctypes library: records, answers `status`, fills the outputs"""

    def __init__(self, status, given):
        self.status, self.given, self.calls = status, given, []

    def __getattr__(self, name):
        return partial(self._call, name)

    def _argument(self, name, pos, a):
        if a is None:
            return 'NULL' if pos else 'ctx'
        arr = getattr(a, '_arr', None)
        if arr is None:
            if hasattr(a, '_length_'):                         # the ctypes array of scfgp_get_dims
                return [type(a)._type_.__name__, a._length_]
            return describe(a)
        rec = {'dtype': str(arr.dtype), 'shape': list(arr.shape), 'contiguous': bool(arr.flags.c_contiguous)}
        if pos not in OUTPUTS[name]:
            rec['values'] = values(arr)
            for k, g in self.given.items():
                if isinstance(g, np.ndarray) and g.size and arr.size and np.shares_memory(arr, g):
                    rec['is' if arr is g else 'of'] = k
        return rec

    def _call(self, name, *args):
        if name == 'scfgp_last_error':
            return ERROR_TEXT.encode()
        assert len(args) == len(_lib.SIGNATURES[name][1]), name
        self.calls.append([name] + [self._argument(name, i, a) for i, a in enumerate(args)])
        if name == 'scfgp_get_dims':
            for i in range(args[1]._length_):
                args[1][i] = T if i == 7 else 100 + i
            return 0
        if self.status in (0, -4):
            for p in OUTPUTS[name]:
                if args[p] is not None:
                    arr = args[p]._arr
                    assert arr.flags.c_contiguous and arr.flags.writeable
                    arr.reshape(-1)[:] = 1000 * p + np.arange(arr.size)
        return self.status


def engine(status=0, nonfinite='raise', scaler=False, given=None):
    e = HipEngine.__new__(HipEngine)
    e.D, e.S, e.M = D, S, M
    e.J = S + M
    e.K = K
    e.P = 3 + D * S + M * S + S + M
    e.ctx = None
    e._pool = {}
    e.nonfinite = nonfinite
    e.lib = Double(status, given or {})
    if scaler:
        e._xcols = list(XCOLS)
    return e


def run(method, kw, status=0, nonfinite='raise', scaler=False, brief=False):
    """one scenario: the record the fixture holds for it"""
    e = engine(status, nonfinite, scaler, kw)
    rec = OrderedDict()
    try:
        rec['returns'] = describe(getattr(e, method)(**kw))
    except Exception as ex:                                    # the type and text are the record
        rec['raises'] = [type(ex).__name__, str(ex)]
    rec['calls'] = [c[0] for c in e.lib.calls] if brief else e.lib.calls
    return rec


# -- inputs: small multiples of 1/8, exact in float32 too -------------------------------------------------------------------------------
def arr(shape, k):
    n = int(np.prod(shape))
    return (((np.arange(n) * 7 + k) % 23 - 11) * 0.125).reshape(shape)


def rows(raw, n=T, k=0):
    return arr((n, D_RAW if raw else D), k)


ALPHA, LI = arr((K, 1), 3), arr((K, K), 5)
W_LIST = [1.0, 0.0, 2.0, 1.0, 0.5]

# method -> (name of its pool rows, its mode names; True / False: a `raw` flag), in the order of engine.py
METHODS = OrderedDict([
    ('predict', ('Xs', None)), ('predict_raw', ('Xs_raw', None)), ('predict_y', ('Xs_raw', None)),
    ('predict_grad', ('Xs', ('scaled', 'raw', 'y'))), ('predict_gradcov', ('Xs', ('scaled', 'raw'))), ('predict_pd', ('Xs', ('scaled', 'raw'))),
    ('sample_weights', (None, None)), ('sample', ('Xs', ('scaled', 'raw', 'y'))), ('sample_argmax', ('Xs', ('scaled', 'raw', 'y'))),
    ('acquire', ('Xs', ('scaled', 'raw'))), ('acquire_kg', ('Xc', ('scaled', 'raw'))), ('sample_grad', ('Xs', ('scaled', 'raw', 'y'))),
    ('predict_cov', ('Xa', ('scaled', 'raw'))), ('condition', ('Xn', ('scaled', 'raw'))), ('forget', ('X', ('scaled', 'raw'))),
    ('loo', ('X', ('scaled', 'raw'))), ('select', ('Xc', (False, True))), ('select_iv', ('Xc', (False, True))),
    ('select_qei', ('Xc', ('scaled', 'raw'))),
])
KINDS = ('ucb', 'pi', 'ei', 'logei', 'mes')
RAW_ONLY = ('predict_raw',)                                    # rows are raw whatever else is said


def is_raw(method, mode):
    return method in RAW_ONLY or mode not in (None, False, 'scaled')


def base(method, mode=None, kind='ei'):
    """keyword arguments of the plain accepted call"""
    xname, modes = METHODS[method]
    raw = is_raw(method, mode)
    kw = OrderedDict()
    if xname:
        kw[xname] = rows(raw)
    if method in ('condition', 'forget', 'loo'):
        kw['yn' if method == 'condition' else 'y'] = arr((T, 1), 1)
    if method == 'sample_grad':
        kw['W'] = arr((K, 3), 2)
    elif method in ('predict_cov', 'select', 'select_iv'):
        kw['Li'] = LI
    else:
        kw['alpha'] = ALPHA; kw['Li'] = LI
    if method == 'predict_pd':
        kw['dims'] = [2, 0] if not raw else [3, 0]
        kw['grid'] = arr((2, 3), 4)
    if method in ('sample_weights', 'sample', 'sample_argmax'):
        kw['nsamp'] = 3
    if method == 'acquire':
        kw['kind'] = kind
        if kind == 'ucb':
            kw['beta'] = 2.0
        elif kind == 'mes':
            kw['fstar'] = arr((3,), 6)
        else:
            kw['best'] = 0.5
    if method in ('select', 'select_iv'):
        kw['m'] = 2
        if mode:
            kw['raw'] = True
    if method == 'select_qei':
        kw['m'] = 2; kw['nsamp'] = 3; kw['best'] = 0.25
    if modes and modes[0] == 'scaled' and mode not in (None, 'scaled'):
        kw['mode'] = mode
    return kw


def full(method, mode=None, kind='ei'):
    """the same with every optional input given and every optional output asked for"""
    raw = is_raw(method, mode)
    kw = base(method, mode, kind)
    opt = {
        'predict_y': dict(ys=arr((T,), 7)),
        'predict_grad': dict(want_std=False),
        'predict_gradcov': dict(w=arr((T,), 8) + 2.0, want=HipEngine.GRADCOV_OUTPUTS),
        'predict_pd': dict(w=arr((T,), 8) + 2.0, want=HipEngine.PD_OUTPUTS),
        'sample_weights': dict(seed=-3),
        'sample': dict(seed=2 ** 64 + 5, noise=True),
        'sample_argmax': dict(seed=-3, w=arr((T,), 8) + 2.0, minimize=True),
        'acquire': dict(xi=0.125, w=arr((T,), 8) + 2.0, noise=True, minimize=True, want=HipEngine.ACQUIRE_WANT),
        'acquire_kg': dict(Xr=rows(raw, R, 9), z=np.linspace(-2.0, 2.0, 5), w=arr((T,), 8) + 2.0, noise=False, minimize=True,
                           want=HipEngine.KG_WANT),
        'sample_grad': dict(sidx=[2, 0, 1, 1, 0], want_val=False),
        'predict_cov': dict(Xb=rows(raw, R, 9)),
        'forget': dict(predict=True),
        'loo': dict(block=2),
        'select': dict(w=arr((T,), 8) + 2.0, return_std=True),
        'select_iv': dict(Xr=rows(raw, R, 9), w=arr((T,), 8) + 2.0, wr=arr((R,), 10) + 2.0, return_std=True),
        'select_qei': dict(xi=0.125, seed=-3, w=arr((T,), 8) + 2.0, pending=rows(raw, R, 9), minimize=True, return_score0=True,
                           return_state=True),
    }
    kw.update(opt.get(method, {}))
    return kw


def scenarios():
    """name -> (method, keyword arguments, keyword arguments of run)"""
    sc = OrderedDict()

    def add(name, method, kw, **how):
        assert name not in sc, name
        sc[name] = (method, kw, how)

    def tag(mode):
        return '' if mode is None else '/%s' % ({False: 'scaled', True: 'raw'}.get(mode, mode),)

    # accepted calls
    for method, (xname, modes) in METHODS.items():
        for mode in modes or (None,):
            for kind in KINDS if method == 'acquire' else (None,):
                name = method + tag(mode) + ('/' + kind if kind else '')
                sc_raw = is_raw(method, mode)
                add('ok/' + name, method, base(method, mode, kind), scaler=sc_raw)
                add('full/' + name, method, full(method, mode, kind), scaler=sc_raw)
        if xname:
            raw = method in RAW_ONLY
            kw = base(method, None)
            wide = np.asarray(np.repeat(rows(raw), 2, axis=1), dtype=np.float32)
            kw[xname] = wide[:, ::2]
            if method in ('predict_gradcov', 'predict_pd', 'sample_argmax', 'acquire', 'acquire_kg', 'select', 'select_iv', 'select_qei'):
                kw['w'] = list(W_LIST)
            add('cast/' + method, method, kw, scaler=raw)
    add('ok/predict_y/scaler', 'predict_y', base('predict_y', 'raw'), scaler=True)
    add('full/predict_y/scaler', 'predict_y', full('predict_y', 'raw'), scaler=True)
    add('ok/condition/estimate', 'condition', {})
    add('ok/forget/predict_only', 'forget', dict(base('forget'), factors=False, predict=True))
    add('ok/loo/resident', 'loo', dict(alpha=ALPHA, Li=LI))
    add('ok/select_qei/no_pending', 'select_qei', dict(base('select_qei'), pending=np.empty((0, D))))
    add('ok/select_iv/wr_of_pool', 'select_iv', dict(base('select_iv'), wr=arr((T,), 10) + 2.0))
    add('ok/acquire/want_str', 'acquire', dict(base('acquire'), want='mu'))
    add('ok/acquire_kg/want_str', 'acquire_kg', dict(base('acquire_kg'), want='kg_hi'))
    add('ok/predict_gradcov/want_str', 'predict_gradcov', dict(base('predict_gradcov'), want='dcov'))
    add('ok/predict_pd/want_str', 'predict_pd', dict(base('predict_pd'), want='ice'))

    # refusals: one faulty argument each
    def bad(name, method, md=None, scaler=None, **change):
        kw = base(method, md)
        for k, v in change.items():
            if v is DROP:
                kw.pop(k)
            else:
                kw[k] = v
        add('bad/%s/%s' % (method, name), method, kw, scaler=is_raw(method, md) if scaler is None else scaler)

    DROP = object()
    for method, (xname, modes) in METHODS.items():
        if modes and modes[0] == 'scaled':
            bad('mode', method, mode='polar')
            for mode in modes[1:]:
                bad('no_scaler_%s' % mode, method, md=mode, scaler=False)
        elif modes:
            bad('no_scaler', method, md=True, scaler=False)
        if xname and method not in ('predict_raw', 'predict_y'):
            bad('rows_1d', method, **{xname: arr((D,), 0)})
            bad('rows_cols', method, **{xname: arr((T, D - 1), 0)})
        if 'w' in full(method):
            bad('w_len', method, w=arr((T + 1,), 8))
        if method == 'sample_grad':
            continue
        if method in ('predict_raw', 'predict_y'):             # they check no shapes
            continue
        if 'alpha' in base(method):
            bad('alpha_shape', method, alpha=arr((K + 1, 1), 3))
        bad('Li_shape', method, Li=arr((K, K + 1), 5))
    bad('rows_f32', 'predict', Xs=np.asarray(rows(False), dtype=np.float32))
    bad('rows_list', 'predict', Xs=rows(False).tolist())
    bad('ys_len', 'predict_y', scaler=False, ys=arr((T + 1,), 7))
    for method in ('predict_gradcov', 'predict_pd'):
        bad('want_name', method, want=('asub', 'pd', 'nope'))
        bad('want_empty', method, want=())
    for method in ('acquire', 'acquire_kg'):
        bad('want_name', method, want=('acq', 'kg', 'nope'))
    bad('dims_dropped', 'predict_pd', md='raw', dims=[1, 0])
    bad('dims_missing', 'predict_pd', md='raw', dims=[0, 6])
    bad('grid_1d', 'predict_pd', grid=arr((3,), 4))
    bad('grid_rows', 'predict_pd', grid=arr((3, 3), 4))
    bad('kind', 'acquire', kind='poi')
    for kind in ('pi', 'ei', 'logei'):
        add('bad/acquire/no_best_%s' % kind, 'acquire', dict(base('acquire', None, 'ucb'), kind=kind))
    add('bad/acquire/no_beta', 'acquire', dict(base('acquire'), kind='ucb'))
    for method in ('acquire_kg', 'select_iv'):
        bad('Xr_1d', method, Xr=arr((D,), 9))
        bad('Xr_cols', method, Xr=arr((R, D + 1), 9))
    bad('wr_len', 'select_iv', Xr=rows(False, R, 9), wr=arr((T,), 10))
    bad('wr_len_pool', 'select_iv', wr=arr((R,), 10))
    bad('pending_1d', 'select_qei', pending=arr((D,), 9))
    bad('pending_cols', 'select_qei', pending=arr((R, D + 1), 9))
    bad('W_1d', 'sample_grad', W=arr((K,), 2))
    bad('W_rows', 'sample_grad', W=arr((K + 1, 3), 2))
    bad('sidx_len', 'sample_grad', sidx=[0, 1])
    bad('Xb_1d', 'predict_cov', Xb=arr((D,), 9))
    bad('Xb_cols', 'predict_cov', Xb=arr((R, D + 1), 9))
    bad('Xb_empty', 'predict_cov', Xb=np.empty((0, D)))
    for method, yname in (('condition', 'yn'), ('forget', 'y'), ('loo', 'y')):
        bad('y_len', method, **{yname: arr((T + 1, 1), 1)})
    for k in ('Xn', 'yn', 'alpha', 'Li'):
        bad('no_' + k, 'condition', **{k: DROP})
    for k in ('X', 'y', 'alpha', 'Li'):
        bad('no_' + k, 'forget', **{k: None})
        bad('no_' + k, 'loo', **{k: None})
    bad('nothing', 'forget', factors=False)

    # counts outside the library's range: the call is still made, with empty outputs; the library answers -1
    def out_of_range(name, method, **change):
        for status in (-1, 0):
            add('range/%s/%s/rc%d' % (method, name, status), method, dict(full(method), **change), status=status)

    for n in (-1, 0, 1025):
        out_of_range('nsamp%d' % n, 'sample', nsamp=n)
    out_of_range('nsamp0', 'sample_weights', nsamp=0)
    for n in (0, 1025):
        out_of_range('nsamp%d' % n, 'sample_argmax', nsamp=n)
        out_of_range('nsamp%d' % n, 'select_qei', nsamp=n)
    for n in (0, 4097):
        for method in ('select', 'select_iv', 'select_qei'):
            out_of_range('m%d' % n, method, m=n)
    for n in (2, 33):
        out_of_range('J%d' % n, 'acquire_kg', z=np.linspace(-1.0, 1.0, n))
    out_of_range('Tb32769', 'predict_cov', Xb=np.zeros((32769, D)))

    # every status, under both settings of nonfinite
    plain = [(m, m, base(m)) for m in METHODS] + [('condition_estimate', 'condition', {}), ('loo_resident', 'loo', dict(alpha=ALPHA, Li=LI))]
    for name, method, kw in plain:
        for status in STATUSES:
            for nonfinite in ('raise', 'return'):
                add('rc/%s/%d/%s' % (name, status, nonfinite), method, kw, status=status, nonfinite=nonfinite, scaler=method in RAW_ONLY,
                    brief=True)
    return sc


def build():
    return OrderedDict((name, run(method, kw, **how)) for name, (method, kw, how) in scenarios().items())


def dumps(records):
    """one scenario per line"""
    return '{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v)) for k, v in records.items()) + '\n}\n'


if __name__ == '__main__':
    records = build()
    with open(PATH, 'w') as f:
        f.write(dumps(records))
    kinds = OrderedDict()
    for name in records:
        kinds[name.split('/')[0]] = kinds.get(name.split('/')[0], 0) + 1
    print('wrote %s: %s, %d bytes' % (PATH, ', '.join('%d %s' % (n, k) for k, n in kinds.items()), os.path.getsize(PATH)))
