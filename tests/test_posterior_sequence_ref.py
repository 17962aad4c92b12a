"""CPU tier of the stale-state sequences (tests/posterior_sequence.py): every schedule the GPU tier uses meets the coverage conditions;
each runs through the runner with the CPU references standing in for the context and for its twins, so the plumbing of every check is
proven without a GPU; no forget step drifts toward a singular downdate; and neither check is vacuous -- one ulp in one element of any
output fails the twin comparison, and an output moved by ten times the bound of its check fails the comparison with the reference."""
import numpy as np
import pytest

from tests import posterior_sequence as PS

IDS = ['%d-%d-%d-%s' % (g + (dt,)) for g, dt in PS.CASES]
MOVED = {}                  # case -> entry points of which an output was moved by ten times its bound


def test_schedules_meet_the_coverage_conditions():
    scheds = PS.check_all_schedules()
    assert len(scheds) == 8
    for ci, steps in enumerate(scheds):
        info = PS.check_schedule(steps, ci)
        print(IDS[ci], info)
        assert set(info['count']) == set(PS.POSTERIOR) and min(info['count'].values()) >= 2 and info['stale'] >= 5
        nsamp = {st['nsamp'] for st in steps if st['op'] == 'post'}; picks = {st['m'] for st in steps if st['op'] == 'post'}
        assert nsamp <= set(PS.NSAMP) and picks <= set(PS.PICKS)
        assert all(1 <= st['block'] <= 64 for st in steps if st['op'] == 'post')
    # the schedules are a function of the case alone
    PS.make_schedule.cache_clear()
    assert PS.make_schedule(3) == scheds[3]
    # across the cases: both forms of loo and of predict_cov, pending rows, masks, all three modes, every sample and pick count
    post = [st for s in scheds for st in s if st['op'] == 'post']
    assert {st.get('resident') for st in post if st['ep'] == 'loo'} == {True, False}
    assert {st['flag'] for st in post if st['ep'] == 'predict_cov'} == {True, False}
    assert {st['flag'] for st in post if st['ep'] == 'select_qei'} == {True, False}
    assert {st['mode'] for st in post} == {'scaled', 'raw', 'y'}
    assert {st['nsamp'] for st in post} == set(PS.NSAMP) and {st['m'] for st in post if st['ep'].startswith('select')} == set(PS.PICKS)
    for ep in PS.Y_MODE + ('predict_y',):
        assert any(st['ep'] == ep and st['mode'] == 'y' for st in post), ep


def _ulp(x):
    """x with one element one ulp up (ints: one up); None where there is nothing to move"""
    if x is None or isinstance(x, (bool, np.bool_)):
        return None
    if isinstance(x, dict):
        k = sorted(x)[-1]
        return dict(x, **{k: np.nextafter(float(x[k]), np.inf)})
    a = np.array(x)
    if a.size == 0:
        return None
    if a.dtype.kind != 'f':
        a.ravel()[0] += 1
        return a
    i = np.flatnonzero(np.isfinite(a.ravel()))
    if i.size == 0:
        return None
    a.ravel()[i[-1]] = np.nextafter(a.ravel()[i[-1]], np.inf)
    return a


@pytest.mark.parametrize('ci', range(len(PS.CASES)), ids=IDS)
def test_dry_run_on_the_references_and_neither_check_is_vacuous(ci):
    moved = {'twin': 0, 'bound': {}, 'exact': 0}

    def on_records(i, a, got, recs):
        # (a) one ulp in one element of any output is a difference from the twin
        for k, v in got.items():
            assert PS.same_bits(v, v)
            w = _ulp(v)
            if w is not None:
                assert not PS.same_bits(w, v), (i, a['ep'], k)
                moved['twin'] += 1
        # (b) ten times the bound in one place fails the record; the records pass as they are
        for rec in recs:
            PS.evaluate(rec)
            bad = PS.perturbed(rec)
            if bad is None:
                continue
            with pytest.raises(AssertionError):
                PS.evaluate(bad)
            if rec[1] == 'exact':
                moved['exact'] += 1
            else:
                moved['bound'][a['ep']] = moved['bound'].get(a['ep'], 0) + 1

    run = PS.Runner(ci, lambda D, S, M, dtype: PS.RefEngine(D, S, M, dtype), on_records=on_records)
    counts = run.run()
    run.close()
    print(IDS[ci], counts, moved, 'min M_ii^2 of the forget steps', run.min_pivot2)
    steps = PS.make_schedule(ci)
    assert counts['twin'] == sum(st['op'] == 'post' for st in steps) and counts['failing'] == sum(st['op'] == 'fail' for st in steps)
    # no schedule drifts toward a singular downdate, where no precision holds (removing a third of the rows leaves about 2/3)
    assert len(run.min_pivot2) >= 2 and min(run.min_pivot2) >= 0.25
    assert moved['twin'] >= counts['twin'] and moved['exact'] > 0
    # an entry point whose only bounded outputs in this schedule were non-finite (predict_y on one row under an inv-normal y scaler) has
    # nothing to move here: the union over the cases is asserted below
    assert len(set(PS.POSTERIOR) - set(moved['bound'])) <= 1, sorted(set(PS.POSTERIOR) - set(moved['bound']))
    MOVED[ci] = set(moved['bound'])


def test_every_entry_point_had_an_output_moved_by_ten_times_its_bound():
    """over the cases that ran before this test in the session (all eight in a full run)"""
    if len(MOVED) == len(PS.CASES):
        assert set.union(*MOVED.values()) == set(PS.POSTERIOR) | {'predict'}
        assert all(sum(ep in m for m in MOVED.values()) >= 4 for ep in PS.POSTERIOR)


def test_failing_calls_raise_the_documented_errors_on_the_references():
    """the three kinds of failing step as the runner makes them: the exception type of each, and nothing raised by a valid call"""
    steps = PS.make_schedule(0)
    kinds = {st['err'] for st in steps if st['op'] == 'fail'}
    assert kinds == {'nonfinite', 'notpd', 'arg'}
    assert PS.ERRORS['nonfinite'][0] is FloatingPointError and PS.ERRORS['notpd'][0] is np.linalg.LinAlgError and PS.ERRORS['arg'][0] is ValueError
