"""
The argument marshalling of scfgp_amd.engine.HipEngine, pinned on the CPU: every posterior and pool method (predict .. select_qei, and
condition() without arguments) is driven with a recording double in place of the shared library, and the call it makes, what it returns
and what it refuses must equal tests/golden/engine_calls.json, the record of the engine.py the fixture was generated from
(tests/golden/make_engine_calls.py holds the double and the scenarios).  Needs neither a GPU nor libscfgp_hip.so.

The second half pins scfgp_amd.model.SCFGP's refusal of a pred_func that is not the library's.
"""
import json

import numpy as np
import pytest

from scfgp_amd.model import SCFGP
from tests.golden import make_engine_calls as G

SCENARIOS = G.scenarios()
with open(G.PATH) as f:
    FIXTURE = json.load(f)


def test_fixture_and_scenarios_name_each_other():
    assert sorted(FIXTURE) == sorted(SCENARIOS)


def test_every_method_and_kind_of_scenario_is_there():
    methods = {method for method, _, _ in SCENARIOS.values()}
    assert methods == set(G.METHODS)
    for kind in ('ok', 'full', 'cast', 'bad', 'range', 'rc'):
        assert any(name.startswith(kind + '/') for name in SCENARIOS)
    for name, rec in FIXTURE.items():                          # what the kinds mean
        if name.startswith('bad/'):
            assert 'raises' in rec and rec['calls'] == [], name
        if name.startswith(('ok/', 'full/', 'range/')):
            assert rec['calls'], name
        if name.startswith(('ok/', 'full/')):
            assert 'returns' in rec, name


@pytest.mark.parametrize('name', sorted(set(SCENARIOS) | set(FIXTURE)))
def test_scenario(name):
    assert name in SCENARIOS and name in FIXTURE
    method, kw, how = SCENARIOS[name]
    got = json.loads(json.dumps(G.run(method, kw, **how)))     # tuples -> lists, as the fixture holds them
    assert got == FIXTURE[name]


@pytest.mark.parametrize('method', [m for m, (xname, _) in G.METHODS.items() if xname and m != 'predict_raw'])
def test_contiguous_float64_rows_are_not_copied(method):
    """the library reads the caller's own array: no copy on the way (predict_raw selects columns, so it always copies)"""
    xname = G.METHODS[method][0]
    kw = G.base(method)
    e = G.engine(given=kw)
    seen = []
    e.lib._argument = lambda name, pos, a: seen.append(getattr(a, '_arr', None))
    getattr(e, method)(**kw)
    assert seen[1] is kw[xname]                                # argument 1 of every one of these entry points is the row array


@pytest.mark.parametrize('method', ['sample_argmax', 'acquire', 'select_qei'])
def test_contiguous_float64_factors_and_weights_are_views(method):
    kw = dict(G.base(method), w=G.arr((G.T,), 8) + 2.0)
    rec = G.run(method, kw)
    owners = [a.get('is') or a.get('of') for a in rec['calls'][-1][1:] if isinstance(a, dict) and 'values' in a]
    assert {'alpha', 'Li', 'w'} <= set(owners)


# -- model.py: the methods that need the library's pred_func -----------------------------------------------------------------------------
def _plain_pred_func(Xs, alpha, Li):
    return None


X5, Y5 = np.zeros((5, 4)), np.zeros((5, 1))
MODEL_CALLS = [
    ('predict_grad', lambda m: m.predict_grad(X5)),
    ('predict_gradcov', lambda m: m.predict_gradcov(X5)),
    ('active_subspace', lambda m: m.active_subspace(X5)),
    ('partial_dependence', lambda m: m.partial_dependence(X5)),
    ('sample', lambda m: m.sample(X5, 3)),
    ('sample_argmax', lambda m: m.sample_argmax(X5, 3)),
    ('sample_maximize', lambda m: m.sample_maximize(X5, 3)),
    ('acquire', lambda m: m.acquire(X5, 'ei')),
    ('kg', lambda m: m.kg(X5)),
    ('mes', lambda m: m.mes(X5, 3)),
    ('acquire_maximize', lambda m: m.acquire_maximize(X5, 'ei')),
    ('predict_cov', lambda m: m.predict_cov(X5)),
    ('condition', lambda m: m.condition(X5, Y5)),
    ('forget', lambda m: m.forget(X5, Y5)),
    ('cv', lambda m: m.cv()),
    ('loo', lambda m: m.loo()),
    ('select', lambda m: m.select(X5, 2)),
    ('select_iv', lambda m: m.select_iv(X5, 2)),
    ('select_qei', lambda m: m.select_qei(X5, 2)),
]


@pytest.mark.parametrize('name,call', MODEL_CALLS, ids=[c[0] for c in MODEL_CALLS])
def test_model_refuses_a_foreign_pred_func(name, call):
    model = SCFGP(sparsity=2, nfeats=3)
    model.pred_func = _plain_pred_func
    with pytest.raises(TypeError) as info:
        call(model)
    assert type(info.value) is TypeError
    assert str(info.value) == "%s needs the library's pred_func (build_hip_models / fit); got %s" % (name, repr(_plain_pred_func))
