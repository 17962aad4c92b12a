"""bench.py's command line and its output dump, without a GPU."""
import os

import numpy as np

import bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse_args(['--steps', '7', '--warmup', '2'])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(['--full', '--dump-outputs', 'out'])
    assert a.full and a.dump_outputs == 'out'


def test_dump_writes_every_output_whole_when_it_fits(tmp_path):
    rng = np.random.default_rng(5)
    arrays = [('cost', np.array([1.25])), ('grad', rng.random(300)), ('alpha', rng.random((40, 1))), ('Li', rng.random((40, 40)))]
    names = bench.dump_outputs(str(tmp_path), arrays)
    assert names == ['Li', 'alpha', 'cost', 'grad']
    for name, v in arrays:
        got = np.load(os.path.join(str(tmp_path), name + '.npy'))
        assert got.dtype == np.float64 and np.array_equal(got, v)


def test_dump_samples_the_largest_output_within_the_limit_and_repeats(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 3 << 20)                 # 1 MiB of it is kept for headers
    rng = np.random.default_rng(6)
    Li = rng.random((600, 600))                                       # 2.75 MiB: does not fit
    arrays = [('cost', np.array([2.5])), ('grad', rng.random(1000)), ('Li', Li)]
    runs = []
    for sub in ('a', 'b'):
        d = os.path.join(str(tmp_path), sub)
        assert bench.dump_outputs(d, arrays) == ['Li', 'Li_index', 'cost', 'grad']
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 3 << 20
        runs.append({f: np.load(os.path.join(d, f)) for f in os.listdir(d)})
    idx = runs[0]['Li_index.npy'].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and 0 < len(idx) < Li.size
    assert np.array_equal(runs[0]['Li.npy'], Li.ravel()[idx])
    assert np.array_equal(runs[0]['grad.npy'], arrays[1][1])
    assert all(np.array_equal(runs[0][f], runs[1][f]) for f in runs[0])
