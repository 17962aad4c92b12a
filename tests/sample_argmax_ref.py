"""
numpy restatement of the per-sample maximisers (include/scfgp_hip.h: scfgp_sample_argmax), on top of tests/sample_ref.py:

    out (T, nsamp): the sample functions at the pool rows (sample_ref.samples, or the library's own scfgp_sample output)
    row t is eligible iff w is None or w[t] > 0
    idx[s] = the lowest eligible t at which out[t][s] is largest (minimize: smallest),   val[s] = out[idx[s]][s]

and the one merge rule that the device applies at every level (lanes, waves, workgroups, launches, chunks, ranks): record a = (v, t)
beats b iff key(a) > key(b), or the keys are equal and a.t < b.t, with key = v, or -v when minimising.
"""
import numpy as np


def beats(a, b, minimize=False):
    """does record a = (v, t) beat record b"""
    ka, kb = (-a[0], -b[0]) if minimize else (a[0], b[0])
    return ka > kb or (ka == kb and a[1] < b[1])


def beats_without_tie_break(a, b, minimize=False):
    """the mutation that test_sample_argmax_ref.py must catch: plain > on the key"""
    ka, kb = (-a[0], -b[0]) if minimize else (a[0], b[0])
    return ka > kb


def merge(records, minimize=False, rule=beats):
    """the winner of a non-empty sequence of records, folded in the order given"""
    best = None
    for r in records:
        if best is None or rule(r, best, minimize):
            best = r
    return best


def argmax(out, w=None, minimize=False):
    """(idx (nsamp,) int64, val (nsamp,)) of the (T, nsamp) block `out` over the eligible rows"""
    out = np.asarray(out, np.float64)
    rows = np.arange(out.shape[0]) if w is None else np.flatnonzero(np.asarray(w) > 0)
    if rows.size == 0:
        raise ValueError('no row has a positive weight')
    sub = out[rows]
    pos = np.argmin(sub, axis=0) if minimize else np.argmax(sub, axis=0)      # numpy: the first occurrence, i.e. the lowest row
    idx = rows[pos].astype(np.int64)
    return idx, out[idx, np.arange(out.shape[1])]


def thompson(out, w=None, minimize=False):
    """SCFGP.thompson's rounds on the (T, m) block `out` of m sample functions: (held (m,) int64, first (m,) int64) with held[s] the row
    that sample s ends up with and first[s] the row it named in round 1.  Round 1 is the plain argmax; among samples that name the same
    row the lowest-numbered keeps it; each further round masks the rows held so far and resolves the samples still without a row by
    the same rule."""
    out = np.asarray(out, np.float64)
    T, m = out.shape
    w = np.ones(T) if w is None else np.array(w, np.float64)
    if m > np.count_nonzero(w > 0):
        raise ValueError('m = %d but only %d rows are eligible' % (m, np.count_nonzero(w > 0)))
    held = np.full(m, -1, np.int64)
    first = None
    while (held < 0).any():
        idx, _ = argmax(out, w, minimize)
        if first is None:
            first = idx.copy()
        for s in np.flatnonzero(held < 0):
            if idx[s] not in held:
                held[s] = idx[s]
        w[held[held >= 0]] = 0.0
    return held, first
