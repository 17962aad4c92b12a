"""CPU tier of the stale-state sequences (tests/posterior_sequence.py): every schedule the GPU tier uses meets the coverage conditions;
each runs through the runner with the CPU references standing in for the context and for its twins, so the plumbing of every check is
proven without a GPU; no forget step drifts toward a singular downdate; and neither check is vacuous -- one ulp in one element of any
output fails the twin comparison, and an output moved by ten times the bound of its check fails the comparison with the reference; every
acquire_kg step meets kg_conditioning and every predict_pd step with sums pd_cancellation, as drawn at run time; and the steps of the
fifteen older entry points are, dict for dict and in their order, the schedules as they stood before the last three joined."""
import zlib

import numpy as np
import pytest

from tests import posterior_sequence as PS

IDS = ['%d-%d-%d-%s' % (g + (dt,)) for g, dt in PS.CASES]
MOVED = {}                  # case -> entry points of which an output was moved by ten times its bound
USED = {}                   # case -> (entry point, T, draw, noise, nodes, R, spread) of the steps drawn at run time, as they ran
# the schedules as they stood before predict_gradcov, predict_pd and acquire_kg joined, per case: the number of steps, the seeds of the
# head's parameters and rows, and the CRC-32 of repr([sorted(step.items()) for step in schedule])
OLD_STEPS = [(63, 1731157065, 303861298, 1792727000), (66, 1578188735, 1690856274, 1631044996), (65, 1601338573, 2105200192, 2953041596),
             (65, 847544755, 149730953, 958381069), (63, 1530833746, 265039639, 3704381806), (63, 1642608774, 388338930, 3753797321),
             (63, 1293936329, 1659304303, 645130781), (63, 1030878329, 250392833, 1604551938)]


def test_the_older_steps_are_the_schedules_as_they_stood():
    """every step of the fifteen older entry points, every training call, change and failing call keeps its arguments, its seed and its
    place among the older steps: the new steps (marked `new`) are inserted between them and move no fit"""
    for ci, pin in enumerate(OLD_STEPS):
        steps = PS.make_schedule(ci)
        old = [st for st in steps if not st.get('new')]
        assert (len(old), old[1]['seed'], old[2]['seed'], zlib.crc32(repr([sorted(st.items()) for st in old]).encode())) == pin, ci
        new = [st for st in steps if st.get('new')]
        assert {st['ep'] for st in new} == set(PS.NEWEST) | {'loo', 'sample', 'predict_cov'} and len(new) in (12, 13)
        assert not any(st.get('ep') in PS.NEWEST or 'redraw' in st or 'G' in st for st in old)
        assert all(st['op'] in ('post', 'fail') and st['ep'] not in ('condition', 'forget') for st in new)      # none moves the fit
        assert steps[:3] == old[:3] and steps[-1] == old[-1] and steps[3] == old[3]


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
    # the three entry points that joined last: both modes, with and without weights, both output sets, every grid size, reference rows
    # given and not, and a node set of their own
    assert len(PS.POSTERIOR) == 18 and {'predict_gradcov', 'predict_pd', 'acquire_kg'} <= set(PS.POSTERIOR)
    for ep in ('predict_gradcov', 'predict_pd', 'acquire_kg'):
        mine = [st for st in post if st['ep'] == ep]
        assert {st['mode'] for st in mine} == {'scaled', 'raw'} and {st['mask'] for st in mine} == {True, False}, ep
    assert {st['flag'] for st in post if st['ep'] == 'predict_gradcov'} == {True, False}
    assert {st['flag'] for st in post if st['ep'] == 'predict_pd'} == {True, False}
    assert {st['G'] for st in post if st['ep'] == 'predict_pd'} == set(PS.GRID) | {5}
    assert {st['pdims'] for st in post if st['ep'] == 'predict_pd'} == {'all', 'one'}
    # acquire_kg's noise and nodes may be replaced by a repeated draw: their coverage is asserted on the arguments as they ran, in
    # test_every_entry_point_had_an_output_moved_by_ten_times_its_bound
    assert {st['R'] for st in post if st['ep'] == 'acquire_kg'} == set(PS.KG_REFS)
    assert all(st['R'] > 0 for st in post if st['ep'] == 'acquire_kg' and st['T'] > 700)


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
    moved = {'twin': 0, 'bound': {}, 'exact': 0, 'conditions': 0}
    holder = {}

    def on_records(i, a, got, recs):
        # (a) one ulp in one element of any output is a difference from the twin
        for k, v in got.items():
            assert PS.same_bits(v, v)
            w = _ulp(v)
            if w is not None:
                assert not PS.same_bits(w, v), (i, a['ep'], k)
                moved['twin'] += 1
        # the input conditions of the steps drawn at run time hold for the draw that was used
        if steps[i].get('redraw'):
            assert PS.input_condition(a, holder['run'].fit), (i, a['ep'])
            if a['ep'] == 'acquire_kg':
                assert PS.kg_conditioning(a, holder['run'].fit) <= 1.0
            elif a['ep'] == 'predict_pd' and set(a['want']) - {'ice'}:
                assert PS.pd_cancellation(a, holder['run'].fit) >= PS.PD_CANCEL
            moved['conditions'] += 1
            assert a['draw'] is not None and PS.used_draw(a) in holder['run'].log[i]
            USED.setdefault(ci, []).append((a['ep'], a['T'], a['draw'], a['noise'], a['nodes'], a['R'], a.get('spread', 1.0)))
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

    steps = PS.make_schedule(ci)
    run = PS.Runner(ci, lambda D, S, M, dtype: PS.RefEngine(D, S, M, dtype), on_records=on_records)
    holder['run'] = run
    counts = run.run()
    run.close()
    print(IDS[ci], counts, moved, 'min M_ii^2 of the forget steps', run.min_pivot2)
    assert moved['conditions'] == sum(bool(st.get('redraw')) and st['op'] == 'post' for st in steps) >= 4
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
        # The steps drawn at run time, as they ran.  acquire_kg: both sigmas, every node set, reference rows given and not, and most
        # steps on their first draw (a repeated draw may replace noise and nodes).  predict_pd: at most one step per schedule on a
        # narrowed pool, and none narrower than half the spread.
        kg = [u for us in USED.values() for u in us if u[0] == 'acquire_kg']
        assert {u[3] for u in kg} == {True, False} and {u[4] for u in kg} == set(PS.KG_NODES) and {u[5] for u in kg} == set(PS.KG_REFS)
        assert len(kg) == 16 and sum(u[2] == 0 for u in kg) >= 8 and max(u[2] for u in kg) < 16
        for ci, us in USED.items():
            pd = [u for u in us if u[0] == 'predict_pd']
            assert len(pd) >= 2 and sum(u[6] == 1.0 for u in pd) >= len(pd) - 1 and min(u[6] for u in pd) >= 0.5, (ci, pd)
            assert all((u[2] == 0) == (u[6] == 1.0) for u in pd)


def test_failing_calls_raise_the_documented_errors_on_the_references():
    """the three kinds of failing step as the runner makes them: the exception type of each, and nothing raised by a valid call"""
    steps = PS.make_schedule(0)
    kinds = {st['err'] for st in steps if st['op'] == 'fail'}
    assert kinds == {'nonfinite', 'notpd', 'arg'}
    assert {(st['ep'], st['err']) for st in steps if st['op'] == 'fail'} >= {('predict_gradcov', 'arg'), ('predict_pd', 'nonfinite')}
    assert PS.ERRORS['nonfinite'][0] is FloatingPointError and PS.ERRORS['notpd'][0] is np.linalg.LinAlgError and PS.ERRORS['arg'][0] is ValueError
