"""The alignment entry points' dispatch table: which (band, alignment type, read_bits, text_bits) each one instantiates, and the
status it answers where it has no instantiation.

One batch of random ACGT jobs is packed at every (read_bits, text_bits) in {2, 4, 8} x {2, 8}.  Where a pair is instantiated, every
result (scores, sinks, sources, CIGARs, edit distances) must equal the 8/8 call's on the same symbols -- the 8/8 results are pinned by
the goldens elsewhere -- so every instantiated arm is launched at least once.  Where it is not, the call must raise UNSUPPORTED.  The
band checks are pinned too: the scorers answer a band they do not instantiate with UNSUPPORTED before looking at the batch, the
tracebacks with INVALID after the empty-batch return."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, 1, 4
BANDS = (3, 7, 15, 31)
TYPES = (0, 1, 2)                                                   # GLOBAL, LOCAL, SEMI_GLOBAL
PAIRS = [(r, t) for r in (2, 4, 8) for t in (2, 8)]
ALL6 = {(4, 2), (2, 2), (8, 2), (8, 8), (4, 8), (2, 8)}
FOUR = {(4, 2), (2, 2), (8, 2), (8, 8)}                             # Best2Sink scorers, Myers
STAGED = {(4, 2), (2, 2), (8, 8)}
GOTOH = [(2, 2, 6, -8, -3, -8, -3), (0, 2, 6, -5, -3, -5, -3)]    # local-style and nvBowtie end-to-end
SW = (2, -3, -2, -2)
J, M, PAD = 37, 50, 8                                               # an odd job count: the packed kernels get an odd pair count


@pytest.fixture(scope="module")
def jobs():
    rng = np.random.default_rng(2024)
    G = 4000
    text = rng.integers(0, 4, G, dtype=np.uint8)
    starts = rng.integers(PAD, G - M - PAD, J)
    reads = np.stack([text[s:s + M] for s in starts]).copy()
    mut = rng.random(reads.shape) < 0.06
    reads[mut] = rng.integers(0, 4, int(mut.sum()))
    for k in range(0, J, 5):                                        # a deletion in every fifth read
        p = int(rng.integers(10, M - 10))
        reads[k] = np.concatenate([text[starts[k]:starts[k] + p], text[starts[k] + p + 2:starts[k] + M + 2]])
    reads[J - 1] = rng.integers(0, 4, M)                           # and one unrelated read
    wb = (starts - PAD).astype(np.uint32)
    we = (starts + M + PAD).astype(np.uint32)
    return reads.reshape(-1), text, wb, we


def _batch(amd, orc, jobs, rb, tb, n=None):
    reads, text, wb, we = jobs
    packed_reads = {2: orc.pack2, 4: orc.pack4, 8: lambda x: x}[rb](reads)
    packed_text = {2: orc.pack2, 8: lambda x: x}[tb](text)
    roffs = (np.arange(J + 1) * M).astype(np.uint32)
    n = J if n is None else n
    return amd.AlignmentBatch(packed_reads, rb, roffs, packed_text, tb, wb[:n], we[:n], max_read_len=M)


def _host(out):
    return [None if t is None else t.cpu().numpy() for t in out]


def _status(amd, fn):
    """the status a call answers (OK when it returns)"""
    try:
        fn()
    except amd.NvbioError as e:
        return e.status
    return OK


def _table(amd, orc, jobs, instantiated, call):
    """call(batch) at every pair: equal to 8/8 where instantiated, UNSUPPORTED elsewhere"""
    want = _host(call(_batch(amd, orc, jobs, 8, 8)))
    for rb, tb in PAIRS:
        batch = _batch(amd, orc, jobs, rb, tb)
        if (rb, tb) in instantiated:
            got = _host(call(batch))
            for g, w in zip(got, want):
                assert (g is None and w is None) or np.array_equal(g, w), (rb, tb)
        else:
            assert _status(amd, lambda: call(batch)) == UNSUPPORTED, (rb, tb)


def _gotoh(amd, typ, sv):
    return amd.make_gotoh_aligner(typ, amd.GotohScheme(*sv))


def _sw(amd, typ):
    return amd.make_smith_waterman_aligner(typ, amd.SimpleSmithWatermanScheme(*SW))


@pytest.mark.parametrize("band", BANDS)
def test_banded_scores(amd, orc, jobs, band):
    for typ in TYPES:
        for sv in GOTOH:
            al = _gotoh(amd, typ, sv)
            _table(amd, orc, jobs, ALL6, lambda b: amd.BatchedBandedAlignmentScore(band, al).enact(b))
            _table(amd, orc, jobs, STAGED, lambda b: amd.BatchedBandedAlignmentScore(
                band, al, scheduler=amd.DEVICE_STAGED_THREAD_SCHEDULER).enact(b))
            _table(amd, orc, jobs, FOUR, lambda b: amd.batch_banded_alignment_score_best2(band, al, b, distinct_dist=4))
        sw = _sw(amd, typ)
        _table(amd, orc, jobs, ALL6, lambda b: amd.BatchedBandedAlignmentScore(band, sw).enact(b))


@pytest.mark.parametrize("text_blocking", (False, True))
def test_full_scores(amd, orc, jobs, text_blocking):
    N = M + 2 * PAD
    for typ in TYPES:
        for sv in GOTOH:
            al = _gotoh(amd, typ, sv)
            _table(amd, orc, jobs, ALL6, lambda b: amd.BatchedAlignmentScore(al, text_blocking).enact(b, M, N))
            _table(amd, orc, jobs, FOUR, lambda b: amd.batch_alignment_score_best2(al, b, M, N, distinct_dist=4,
                                                                                    text_blocking=text_blocking))
        sw = _sw(amd, typ)
        _table(amd, orc, jobs, ALL6, lambda b: amd.BatchedAlignmentScore(sw, text_blocking).enact(b, M, N))


def _cigars(out):
    """(scores, sources, sinks, cigars, lens) -> the same with each CIGAR cut at its length"""
    sc, src, sk, cig, ln = out
    keep = np.arange(cig.shape[1])[None, :] < ln.cpu().numpy()[:, None]
    import torch
    return sc, src, sk, cig * torch.as_tensor(keep, device=cig.device), ln


@pytest.mark.parametrize("band", BANDS)
def test_banded_tracebacks(amd, orc, jobs, band):
    for typ in TYPES:
        for al in [_gotoh(amd, typ, sv) for sv in GOTOH] + [_sw(amd, typ)]:
            _table(amd, orc, jobs, ALL6, lambda b: _cigars(amd.BatchedBandedAlignmentTraceback(band, al).enact(b)))


def test_full_tracebacks_and_finish(amd, orc, jobs):
    N = M + 2 * PAD
    for typ in TYPES:
        for al in [_gotoh(amd, typ, sv) for sv in GOTOH] + [_sw(amd, typ)]:
            _table(amd, orc, jobs, ALL6, lambda b: _cigars(amd.BatchedAlignmentTraceback(al).enact(b, M, N)))
    # finish_alignment over one traceback's output, read at every pair
    _, src, _, cig, ln = amd.BatchedAlignmentTraceback(_gotoh(amd, 2, GOTOH[1])).enact(_batch(amd, orc, jobs, 8, 8), M, N)
    _table(amd, orc, jobs, ALL6, lambda b: amd.finish_alignment(b, src, cig, ln, mds_stride=96))


def test_myers(amd, orc, jobs):
    for band in (7, 15, 31):
        for typ in (0, 2):
            _table(amd, orc, jobs, FOUR, lambda b: amd.batch_banded_myers_score(band, typ, b))
    assert _status(amd, lambda: amd.batch_banded_myers_score(15, 1, _batch(amd, orc, jobs, 8, 8))) == INVALID


def test_band_and_type_checks(amd, orc, jobs):
    """a band that is not instantiated, an empty batch, an alignment type that does not exist: the status of every path"""
    import ctypes
    full, empty = _batch(amd, orc, jobs, 4, 2), _batch(amd, orc, jobs, 4, 2, n=0)
    al, sw = _gotoh(amd, 1, GOTOH[0]), _sw(amd, 1)
    scorers = [
        lambda band, b, a=al: amd.BatchedBandedAlignmentScore(band, a).enact(b),
        lambda band, b, a=sw: amd.BatchedBandedAlignmentScore(band, a).enact(b),
        lambda band, b, a=al: amd.BatchedBandedAlignmentScore(band, a, scheduler=amd.DEVICE_STAGED_THREAD_SCHEDULER).enact(b),
        lambda band, b, a=al: amd.batch_banded_alignment_score_best2(band, a, b),
    ]
    tracebacks = [lambda band, b, a=a: amd.BatchedBandedAlignmentTraceback(band, a).enact(b) for a in (al, sw)]
    for band in (0, 5, 16, 32, 63):
        for f in scorers:
            assert _status(amd, lambda: f(band, full)) == UNSUPPORTED, band
            assert _status(amd, lambda: f(band, empty)) == UNSUPPORTED, band          # the band is checked before the empty-batch return
        for f in tracebacks:
            assert _status(amd, lambda: f(band, full)) == INVALID, band
            assert _status(amd, lambda: f(band, empty)) == OK, band                    # ... and after it
        out = ctypes.c_uint64(0)
        assert amd.lib().nvbio_banded_gotoh_traceback_temp_bytes(ctypes.byref(full.c_struct()), ctypes.c_uint32(band),
                                                                 ctypes.byref(out)) == INVALID
    for band in BANDS:
        for f in scorers + tracebacks:
            assert _status(amd, lambda: f(band, empty)) == OK, band
    # an alignment type outside GLOBAL / LOCAL / SEMI_GLOBAL
    N = M + 2 * PAD
    bad = [
        lambda a: amd.BatchedBandedAlignmentScore(31, a).enact(full),
        lambda a: amd.BatchedBandedAlignmentScore(31, a, scheduler=amd.DEVICE_STAGED_THREAD_SCHEDULER).enact(full),
        lambda a: amd.batch_banded_alignment_score_best2(31, a, full),
        lambda a: amd.BatchedBandedAlignmentTraceback(31, a).enact(full),
        lambda a: amd.BatchedAlignmentScore(a, True).enact(full, M, N),
        lambda a: amd.BatchedAlignmentScore(a, False).enact(full, M, N),
        lambda a: amd.batch_alignment_score_best2(a, full, M, N),
        lambda a: amd.BatchedAlignmentTraceback(a).enact(full, M, N),
    ]
    for f in bad:
        assert _status(amd, lambda: f(_gotoh(amd, 3, GOTOH[0]))) == INVALID
