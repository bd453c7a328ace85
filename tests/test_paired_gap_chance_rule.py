"""The pairing rule of the band-31 gap chance (nvbio_banded_gap_pairs, include/nvbio_amd.h), restated in numpy and pinned on hand-written
cases.  tests/test_gpu_band31_paired_gap_chance.py holds the library to this restatement on every batch it scores.

Jobs j and j + 1 are LINKED iff they have the same read and the same flags, both windows are unclipped (win_end - win_begin = read length + 31,
read length 1..161), 0 < |win_begin[j+1] - win_begin[j]| <= 5 (the seed pass hands a read's candidates over in seed order, so either job may hold
the lower window), and j is not the last job of a wave of the first pass (j % 64 != 63).  Along a run
of linked jobs the pairs are taken from its lowest job on; a job left over stays alone."""
import numpy as np

MAX_SHIFT = 5
NO_PARTNER = 0xFFFFFFFF


def gap_pairs(roffs, wb, we, read_id=None, flags=None, max_shift=MAX_SHIFT):
    roffs, wb, we = (np.asarray(a, dtype=np.int64) for a in (roffs, wb, we))
    n = len(wb)
    partner = np.full(n, NO_PARTNER, dtype=np.uint32)
    if read_id is None:                                            # job i is read i: no two jobs share a read
        return partner
    rid = np.asarray(read_id, dtype=np.int64)
    fl = np.zeros(n, dtype=np.int64) if flags is None else np.asarray(flags, dtype=np.int64)
    M = roffs[rid + 1] - roffs[rid]
    whole = (M >= 1) & (M <= 161) & (we - wb == M + 31)
    j = 0
    while j + 1 < n:
        shift = abs(wb[j + 1] - wb[j])
        if (j % 64 != 63 and whole[j] and whole[j + 1] and rid[j] == rid[j + 1] and fl[j] == fl[j + 1] and 0 < shift <= max_shift):
            partner[j], partner[j + 1] = j + 1, j
            j += 2
        else:
            j += 1
    return partner


def _batch(M, jobs):
    """jobs: (read, win_begin, window length or None for M + 31, flags); reads all M long"""
    rid = np.array([j[0] for j in jobs]); wb = np.array([j[1] for j in jobs])
    we = wb + np.array([M + 31 if j[2] is None else j[2] for j in jobs]); fl = np.array([j[3] for j in jobs])
    roffs = np.arange(int(rid.max()) + 2) * M
    return roffs, wb, we, rid, fl


def _p(*pairs_of, n):
    want = np.full(n, NO_PARTNER, dtype=np.uint32)
    for a, b in pairs_of:
        want[a], want[b] = b, a
    return want


def test_shifts_one_to_five_pair_and_six_does_not():
    for s in range(0, 8):
        got = gap_pairs(*_batch(150, [(0, 100, None, 0), (0, 100 + s, None, 0)]))
        assert np.array_equal(got, _p((0, 1), n=2) if 1 <= s <= 5 else _p(n=2)), s
    # the upper window first
    for s in range(0, 8):
        got = gap_pairs(*_batch(150, [(0, 100 + s, None, 0), (0, 100, None, 0)]))
        assert np.array_equal(got, _p((0, 1), n=2) if 1 <= s <= 5 else _p(n=2)), s


def test_read_strand_and_clipping():
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, None, 0), (1, 102, None, 0)])), _p(n=2))            # two reads
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, None, 0), (0, 102, None, 3)])), _p(n=2))            # opposite strands
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, None, 3), (0, 102, None, 3)])), _p((0, 1), n=2))
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, None, 0), (0, 102, 150 + 29, 0)])), _p(n=2))        # upper window clipped
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, 150 + 30, 0), (0, 102, None, 0)])), _p(n=2))        # lower window clipped
    assert np.array_equal(gap_pairs(*_batch(162, [(0, 100, None, 0), (0, 102, None, 0)])), _p(n=2))            # too long for the planes
    assert np.array_equal(gap_pairs(*_batch(161, [(0, 100, None, 0), (0, 105, None, 0)])), _p((0, 1), n=2))
    # without read ids every job is a read of its own
    roffs, wb, we, rid, fl = _batch(150, [(0, 100, None, 0), (0, 102, None, 0)])
    assert np.array_equal(gap_pairs(np.arange(3) * 150, wb, we, None, fl), _p(n=2))


def test_adjacency_and_runs():
    # the same read at a non-adjacent index stays alone
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, None, 0), (1, 500, None, 0), (0, 102, None, 0)])), _p(n=3))
    # three in a row: the lower two pair, the third is single; four in a row: two pairs
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, None, 0), (0, 101, None, 0), (0, 103, None, 0)])), _p((0, 1), n=3))
    assert np.array_equal(gap_pairs(*_batch(150, [(0, 100, None, 0), (0, 101, None, 0), (0, 103, None, 0), (0, 104, None, 0)])), _p((0, 1), (2, 3), n=4))
    # a run that starts after a single job
    assert np.array_equal(gap_pairs(*_batch(150, [(1, 700, None, 0), (0, 100, None, 0), (0, 101, None, 0), (0, 103, None, 0)])), _p((1, 2), n=4))


def test_no_pair_across_a_wave_of_64_jobs():
    jobs = [(9, 5000, None, 0)] + [(r, 1000 * r + 100 + 2 * k, None, 0) for r in range(40) for k in range(2)]
    got = gap_pairs(*_batch(150, jobs))
    want = _p(*[(1 + 2 * r, 2 + 2 * r) for r in range(40) if (1 + 2 * r) % 64 != 63], n=81)
    assert np.array_equal(got, want) and got[63] == NO_PARTNER and got[64] == NO_PARTNER
    # ... and a run that crosses the boundary starts afresh behind it: 62, 63 | 64, 65 linked in a row
    jobs = [(r, 1000 * r, None, 0) for r in range(1, 63)] + [(0, 100 + k, None, 0) for k in range(4)]
    assert len(jobs) == 66
    got = gap_pairs(*_batch(150, jobs))
    assert np.array_equal(got, _p((62, 63), (64, 65), n=66))
    jobs = [(r, 1000 * r, None, 0) for r in range(1, 64)] + [(0, 100 + k, None, 0) for k in range(3)]          # 63, 64, 65 in a row
    assert np.array_equal(gap_pairs(*_batch(150, jobs)), _p((64, 65), n=66))
