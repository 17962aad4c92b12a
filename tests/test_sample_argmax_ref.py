"""CPU tier of scfgp_sample_argmax: the merge rule of tests/sample_argmax_ref.py is independent of how the records are grouped and
ordered (exact ties, both signs, both directions), its mutation without the index tie-break is caught by a duplicated row, the
restated argmax agrees with the rule, and the rounds of thompson return distinct rows that keep round 1's uncontested choices."""
import numpy as np
import pytest

from scfgp_amd import synth
from tests import sample_argmax_ref as A
from tests import sample_ref as R


def _records(rng, n):
    """n records (v, t) with distinct t, values of either sign drawn from a small set so that exact ties are common"""
    v = rng.choice(np.array([-2.5, -1.0, -0.0, 0.0, 0.75, 3.0, 3.0, -2.5]), n) * rng.choice([1.0, 1.0, 0.5], n)
    return [(float(v[i]), int(t)) for i, t in enumerate(rng.permutation(4 * n)[:n])]


def _grouped(rng, recs, minimize, rule=A.beats):
    """merge a random partition of a random order of the records group by group, then the group winners in a random order"""
    recs = [recs[i] for i in rng.permutation(len(recs))]
    cuts = np.sort(rng.choice(np.arange(1, len(recs)), rng.integers(0, min(6, len(recs) - 1) + 1), replace=False))
    groups = [g for g in np.split(np.arange(len(recs)), cuts) if len(g)]
    winners = [A.merge([recs[i] for i in g], minimize, rule) for g in groups]
    return A.merge([winners[i] for i in rng.permutation(len(winners))], minimize, rule)


@pytest.mark.parametrize('minimize', [False, True])
def test_merge_rule_does_not_depend_on_grouping_or_order(minimize):
    rng = np.random.default_rng(11)
    for _ in range(200):
        recs = _records(rng, int(rng.integers(2, 40)))
        key = [(-v if minimize else v) for v, _ in recs]
        top = max(key)
        want = min(t for (v, t), k in zip(recs, key) if k == top)           # the definition: the lowest t among the best keys
        for _ in range(5):
            got = _grouped(rng, recs, minimize)
            assert got[1] == want and (-got[0] if minimize else got[0]) == top


@pytest.mark.parametrize('minimize', [False, True])
def test_argmax_agrees_with_the_merge_rule(minimize):
    rng = np.random.default_rng(12)
    out = rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 2.0]), (60, 9))
    w = (rng.random(60) < 0.7).astype(float) * 3.5
    for wt in (None, w):
        idx, val = A.argmax(out, wt, minimize)
        for s in range(out.shape[1]):
            rows = range(60) if wt is None else np.flatnonzero(wt > 0)
            v, t = A.merge([(float(out[t, s]), int(t)) for t in rows], minimize)
            assert (idx[s], val[s]) == (t, v)
            assert np.signbit(val[s]) == np.signbit(out[idx[s], s])
    with pytest.raises(ValueError):
        A.argmax(out, np.zeros(60), minimize)


@pytest.mark.parametrize('minimize', [False, True])
def test_mutation_without_the_tie_break_is_caught_by_a_duplicated_row(minimize):
    rng = np.random.default_rng(13)
    col = rng.standard_normal(50)
    recs = [(float(v), t) for t, v in enumerate(np.r_[col, col])]              # every row again, 50 rows later: every value ties
    want = int(np.argmin(col) if minimize else np.argmax(col))
    assert A.argmax(np.r_[col, col][:, None], None, minimize)[0][0] == want
    assert all(_grouped(rng, recs, minimize)[1] == want for _ in range(50))
    wrong = [_grouped(rng, recs, minimize, A.beats_without_tie_break)[1] for _ in range(50)]
    assert any(t == want + 50 for t in wrong)                                  # the mutant's answer depends on the order
    assert all(t in (want, want + 50) for t in wrong)


def _sample_block(T, m, seed):
    D, S, M = 3, 1, 20
    K = 2 * (S + M)
    params = synth.make_params(77, D, S, M, abc=(-1.0, 0.0, -1.0))
    rng = np.random.default_rng(78)
    alpha = rng.standard_normal(K) / np.sqrt(K)
    Li = np.tril(rng.standard_normal((K, K))) / np.sqrt(K)
    return R.samples(synth.make_X(79, T, D), alpha, Li, params, S, M, m, seed)


@pytest.mark.parametrize('minimize', [False, True])
def test_thompson_rounds(minimize):
    T, m = 40, 24                                                  # few rows, many samples: contested rows and several rounds
    out = _sample_block(T, m, 5)
    w = np.ones(T); w[[3, 17]] = 0.0
    for wt in (None, w):
        held, first = A.thompson(out, wt, minimize)
        assert np.array_equal(first, A.argmax(out, wt, minimize)[0])
        assert len(set(held.tolist())) == m and held.min() >= 0
        if wt is not None:
            assert not np.isin(held, [3, 17]).any()
        assert len(set(first.tolist())) < m                        # the case does exercise the later rounds
        for s in range(m):
            if first[s] not in first[:s]:                          # no lower sample named it: sample s keeps its round-1 row
                assert held[s] == first[s]
            else:
                assert held[s] != first[s]
    few = np.zeros(T); few[:m - 1] = 1.0
    with pytest.raises(ValueError):
        A.thompson(out, few, minimize)
    held, _ = A.thompson(out[:, :5], np.r_[np.ones(5), np.zeros(T - 5)], minimize)      # as many rows as samples: a permutation
    assert sorted(held.tolist()) == list(range(5))
