"""GPU: every C entry point of the selection stage (csrc/seed_extend.hip: diagonal keys, candidate windows, best / second best / unpack /
MAPQ, the fused finish_reads, the traceback batch, opposite-mate windows, the score stream, the two sw-benchmark conversions) on its own
against the plain-integer restatement of selection_cpu.py, every output array in full, on the lists of selection_cases.py: genome ends and
starts, the 33-bit position field, wave and grid-stride boundaries, ties, rejected candidates, the distinctness rule at its distance.
None of these kernels reads the text, so genome_len may be 0xFFFFFFFF without a genome.  Integer-exact: no tolerance anywhere."""
import itertools

import numpy as np
import pytest

import selection_cases as cases
import selection_cpu as sel

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
M, DIST, MIN_SCORE, WORST, BAND = cases.M, cases.DIST, cases.MIN_SCORE, cases.WORST, cases.BAND


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def _i64(torch, values):
    return torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).cuda()


def _i32(torch, values, dtype=np.uint32):
    return torch.from_numpy(np.array(values, dtype=dtype).view(np.int32)).cuda()


def _device(torch, cands):
    """(keys, scores, sinks, win_begin) of a candidate list"""
    sinks = np.array([[c[3], M] for c in cands], dtype=np.uint32).reshape(-1, 2)
    return (_i64(torch, [c[0] for c in cands]), _i32(torch, [c[1] for c in cands], np.int32), torch.from_numpy(sinks.view(np.int32)).cuda(),
            _i32(torch, [c[2] for c in cands]))


def _u64(t):
    return [int(v) for v in t.cpu().numpy().view(np.uint64)]


def _ints(t):
    return [int(v) for v in t.cpu().numpy()]


def _u32s(amd, t):
    return [int(v) for v in amd.u32(t)]


_LISTS = {}


def _list(name):
    """(cands, n_reads, read lengths) of a named list, and the restatement's best of it, computed once"""
    if name not in _LISTS:
        if name == "runs":
            cands, n_reads = cases.run_list()[:2]
        elif name == "runs-permuted":
            cands, n_reads = cases.permuted_run_list()
        elif name == "edges":
            cands, n_reads = cases.edge_list()[:2]
        else:
            cands, n_reads = cases.random_list(21)
        lengths = cases.edge_list()[3] if name == "edges" else [int(v) for v in np.random.default_rng(len(cands)).integers(100, M + 1, n_reads)]
        _LISTS[name] = (cands, n_reads, lengths, sel.best_per_read(cands, n_reads))
    return _LISTS[name]


# ---- keys -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spr,interval,L,Mr,n_ids", [(13, 10, 22, 150, 100), (1, 1, 22, 150, 40), (2, 1024, 22, 1046, 7)],
                         ids=["13-seeds", "1-seed", "offset-1024"])
def test_hits_to_diagonals(amd, spr, interval, L, Mr, n_ids):
    import torch
    hits = cases.key_hits(spr, interval, L, Mr, n_ids)
    ht = torch.from_numpy(np.array(hits, dtype=np.uint32).view(np.int32)).cuda()
    fields = []
    for strand in (0, 1):
        want = [sel.hit_to_diagonal(t, sid, spr, interval, L, Mr, strand) for t, sid in hits]
        assert _u64(amd.hits_to_diagonals(ht, spr, interval, L, Mr, strand)) == want
        fields += [w & sel.FIELD for w in want]
    assert n_ids % spr != 0 or spr == 1                              # the ids do not fill the last read
    assert min(fields) == sel.BIAS - (Mr - L) and max(fields) == U32 - L + sel.BIAS       # the last seed at position 0; the genome's last seed
    assert (min(fields) == 0) == (Mr - L == sel.MAX_SEED_OFFSET)


def test_key_calls_refuse_reads_beyond_the_seed_offset_limit(amd):
    """read_len - seed_len = 1025: a hit of the last seed at position 0 would leave the field; the call refuses, whatever the hits are.
    (The key calls alone: their outputs are indexed by hit.  No out-of-range key is ever handed to a reducer.)"""
    import torch
    ht = torch.from_numpy(np.array([[5000, 0], [6000, 1]], dtype=np.uint32).view(np.int32)).cuda()
    for strand in (0, 1):
        assert _u64(amd.hits_to_diagonals(ht, 2, 1024, 22, 1046, strand)) == [sel.hit_to_diagonal(t, s, 2, 1024, 22, 1046, strand) for t, s in ((5000, 0), (6000, 1))]
        with pytest.raises(amd.NvbioError, match="NVBIO_MAX_SEED_OFFSET") as e:
            amd.hits_to_diagonals(ht, 2, 1025, 22, 1047, strand)
        assert e.value.status == 1
        with pytest.raises(amd.NvbioError, match="NVBIO_MAX_SEED_OFFSET"):
            amd.hits_to_diagonals(ht, 1, 1, 22, 5000, strand)


def test_locate_diagonals_on_a_small_index(amd, orc):
    """the same keys from nvbio_fm_filter_locate_diagonals: reads cut so that their seeds hit the first symbols of a 400-symbol text, on both strands"""
    import torch
    rng = np.random.default_rng(33)
    n, pad, L, S = 400, 130, 22, 10
    spr = (M - L) // S + 1
    text = rng.integers(0, 4, n, dtype=np.uint8)
    padded = np.concatenate([rng.integers(0, 4, pad, dtype=np.uint8), text])
    # (the last seed lies 120 symbols into the forward read and 128 into the reverse-complemented one: cut there, one before and one after)
    cuts = [pad - 129, pad - 128, pad - 127, pad - 121, pad - 120, pad - 119, pad - 1, pad, pad + 1, pad + 2, pad + 60]
    reads = [padded[k:k + M] for k in cuts]
    reads += [(3 - r[::-1]).astype(np.uint8) for r in reads]
    R = len(reads)
    hidx = orc.build_index(text)
    fmi = amd.FMIndex.from_arrays(hidx.n, hidx.primary, hidx.L2, hidx.bwt_occ, hidx.ssa)
    qs = amd.PackedStringSet(orc.pack4(np.concatenate(reads)), 4, R * spr, fixed_len=L, stride=M, seeds_per_string=spr, seed_interval=S)
    for strand, flags in ((0, 0), (1, amd.FM_SCAN_FORWARD | amd.FM_COMPLEMENT)):
        flt = amd.FMIndexFilter()
        total = flt.rank(fmi, qs, flags)
        assert total >= 4 * spr
        hits = amd.u32(flt.locate(0, total))
        want = [sel.hit_to_diagonal(int(t), int(sid), spr, S, L, M, strand) for t, sid in hits]
        keys = flt.locate_diagonals(0, total, spr, S, L, M, strand)
        assert _u64(keys) == want
        assert torch.equal(keys, amd.hits_to_diagonals(torch.from_numpy(hits.view(np.int32)).cuda(), spr, S, L, M, strand))
        # seeds hanging over the genome start, the last one of a read at position 0 and at position 1
        assert sum(1 for w in want if w & sel.FIELD < sel.BIAS) >= 10 and {0, 1} <= {int(t) for t in hits[:, 0]}
        assert min(w & sel.FIELD for w in want) == sel.BIAS - (128 if strand else 120)
        with pytest.raises(amd.NvbioError, match="NVBIO_MAX_SEED_OFFSET"):
            flt.locate_diagonals(0, total, 2, 1100, L, 1122, strand)
    # the other calls that form keys refuse the same geometry before they launch anything
    long_read = amd.PackedStringSet(orc.pack4(rng.integers(0, 4, 1122, dtype=np.uint8)), 4, 2, fixed_len=L, stride=1122, seeds_per_string=2, seed_interval=1100)
    with pytest.raises(amd.NvbioError, match="NVBIO_MAX_SEED_OFFSET"):
        fmi.match_seed_diagonals(long_read, 0, 1122, 0)
    ranges = torch.tensor([[3, 4]], dtype=torch.int32, device="cuda")
    with pytest.raises(amd.NvbioError, match="NVBIO_MAX_SEED_OFFSET"):
        fmi.residual_diagonals(ranges, torch.tensor([1], dtype=torch.int32, device="cuda"), 4, 2, 1100, L, 1122)
    fmi.close()


def test_two_strand_seed_pass_refuses_reads_beyond_the_seed_offset_limit(amd, orc):
    rng = np.random.default_rng(34)
    G, L = 50_000, 16
    fmi = amd.FMIndex.build(orc.pack2(rng.integers(0, 4, G, dtype=np.uint8)), G, kmer_len=11, sa_int=1, table_flags=amd.FM_TABLE_CANONICAL_WIDE)
    Mr = L + sel.MAX_SEED_OFFSET + 1
    qs = amd.PackedStringSet(orc.pack4(rng.integers(0, 4, Mr, dtype=np.uint8)), 4, 2, fixed_len=L, stride=Mr, seeds_per_string=2, seed_interval=Mr - L)
    with pytest.raises(amd.NvbioError, match="NVBIO_MAX_SEED_OFFSET"):
        fmi.match_seed_diagonals_both(qs, Mr)
    fmi.close()


# ---- windows ----------------------------------------------------------------------------------------------------------------------
RAGGED_LENGTHS = [1, 1023, 150, 149, 7, 100]


def _window_case(band, G):
    """keys on every edge of the window rule for reads of RAGGED_LENGTHS (the edges are placed for each read's own length and for M), and
    a few thousand random ones"""
    rng = np.random.default_rng(band + 1000)
    low = (1 << 34) - 1
    keys = cases.window_keys(band, M, G, len(RAGGED_LENGTHS))
    for r, length in enumerate(RAGGED_LENGTHS):
        keys += [(r << 34) | (k & low) for k in cases.window_keys(band, length, G, 1)]
    fields = rng.integers(0, G + sel.BIAS, 3000, dtype=np.uint64)
    keys += [(int(rng.integers(0, len(RAGGED_LENGTHS))) << 34) | (int(rng.integers(0, 2)) << 33) | int(f) for f in fields]
    return keys


def _check_windows(amd, torch, keys, band, G, ragged):
    off = cases.ragged_of(RAGGED_LENGTHS)[0]
    want = sel.windows(keys, band, M, G, read_offsets=off if ragged else None)
    got = amd.diagonals_to_windows(_i64(torch, keys), band, M, G, read_offsets=_i32(torch, off) if ragged else None)
    assert _u32s(amd, got[0]) == [w[0] for w in want]
    assert _ints(got[1]) == [w[1] for w in want]
    assert _u32s(amd, got[2]) == [w[2] for w in want]
    assert _u32s(amd, got[3]) == [w[3] for w in want]
    return want


@pytest.mark.parametrize("G", [1_000_000, U32], ids=["1M", "4G"])
@pytest.mark.parametrize("band", [0, 1, 30, 31, 32])
def test_diagonals_to_windows(amd, band, G):
    import torch
    keys = _window_case(band, G)
    for ragged in (False, True):
        want = _check_windows(amd, torch, keys, band, G, ragged)
        lens = [RAGGED_LENGTHS[k >> 34] if ragged else M for k in keys]
        fields = [k & sel.FIELD for k in keys]
        assert sum(1 for f in fields if f < sel.BIAS) >= 4 and sum(1 for f in fields if f == sel.BIAS) >= 2            # diagonals below and at 0
        assert sum(1 for f, w in zip(fields, want) if f > sel.BIAS and w[2] == 0) >= 2 * (band > 1)                    # inside the half band
        assert sum(1 for w, m in zip(want, lens) if w[2] + band + m == G) >= 2                                          # the end exactly at the genome's
        assert sum(1 for w, m in zip(want, lens) if w[2] + band + m == G + 1 and w[3] == G) >= 2                        # ... one past it: clamped
        if G == U32:
            assert sum(1 for w, m in zip(want, lens) if w[2] + band + m >= 1 << 32) >= 4
    if band == 31:
        for n in (1, 255, 256, 257):
            _check_windows(amd, torch, keys[:n], band, G, False)
            _check_windows(amd, torch, keys[-n:], band, G, True)


# ---- best and unpack --------------------------------------------------------------------------------------------------------------
def _check_unpack(amd, torch, best):
    score, pos, rc = amd.best_candidate_unpack(_i64(torch, best))
    un = [sel.unpack(b) for b in best]
    assert _ints(score) == [u[0] for u in un]
    assert _ints(pos) == [u[1] for u in un]
    assert _ints(rc) == [u[2] for u in un]


@pytest.mark.parametrize("name", ["runs", "runs-permuted", "edges", "random"])
def test_best_candidate_reduce_and_unpack(amd, name):
    import torch
    cands, n_reads, _, want = _list(name)
    keys, scores, sinks, wb = _device(torch, cands)
    best = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    amd.best_candidate_reduce(keys, scores, sinks, wb, best)
    assert _u64(best) == want
    _check_unpack(amd, torch, want)
    if name.startswith("runs"):
        runs = cases.run_list()[2]
        assert want == _list("runs")[3]                               # the order of the candidates does not matter
        assert sum(1 for _, first, n, _ in runs if first % 64 + n > 64) >= 60 and sum(1 for b in want if b == 0) >= len(runs)
        if name == "runs":
            for rid, first, n, top in runs:
                assert want[rid] == sel.selection_key(*cands[top])
    if name == "edges":
        label = cases.edge_list()[2]
        assert sel.unpack(want[label["field33"]])[1] >= 1 << 32
        assert sel.unpack(want[label["tie"]])[1:] == (10_000 + 5_000 * label["tie"] + 200, 1)
        # a read whose only candidates were rejected: a key that is not 0, score NVBIO_SCORE_MIN, the key's position field and strand
        assert want[label["rej_alone"]] != 0 and sel.unpack(want[label["rej_alone"]]) == (sel.SCORE_MIN, 10_000 + 5_000 * label["rej_alone"] + U32, 1)
        assert [sel.unpack(want[label[k]])[0] for k in ("m20-1", "m20", "m20+1")] == [sel.SCORE_MIN, sel.SCORE_MIN, -(1 << 20) + 1]


def test_best_candidate_reduce_over_the_grid_stride_wrap(amd):
    """2^21 + 321 candidates: the capped grid (8192 blocks of 256) takes its stride loop twice, and a read's run straddles the wrap"""
    import torch
    keys, scores, wb, sx, n_reads = cases.big_list()
    assert len(keys) == cases.BIG_N > 8192 * 256 and keys[8192 * 256 - 1] >> np.uint64(34) == keys[8192 * 256] >> np.uint64(34)
    want = sel.best_per_read_np(keys, sel.selection_keys_np(keys, scores, wb, sx), n_reads)
    sinks = np.stack([sx, np.full_like(sx, M)], axis=1)
    best = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    amd.best_candidate_reduce(torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(sinks.view(np.int32)).cuda(),
                              torch.from_numpy(wb.view(np.int32)).cuda(), best)
    assert np.array_equal(best.cpu().numpy().view(np.uint64), want)
    score, pos, rc = amd.best_candidate_unpack(best)
    ws, wp, wr = sel.unpack_np(want)
    assert np.array_equal(score.cpu().numpy(), ws) and np.array_equal(pos.cpu().numpy(), wp) and np.array_equal(rc.cpu().numpy(), wr)
    assert want[-1] == 0 and (want[:-1] != 0).sum() > 3900


# ---- second best ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("name", ["runs", "runs-permuted", "edges", "random"])
def test_second_candidate_reduce(amd, name, ragged):
    import torch
    cands, n_reads, lengths, best = _list(name)
    off, mins = cases.ragged_of(lengths)
    want = sel.second_per_read(cands, best, DIST, WORST, read_offsets=off if ragged else None, min_scores=mins if ragged else None)
    keys, scores, sinks, wb = _device(torch, cands)
    second = torch.zeros(n_reads, dtype=torch.int64, device="cuda")
    amd.second_candidate_reduce(keys, scores, sinks, wb, _i64(torch, best), DIST, WORST, second,
                                read_offsets=_i32(torch, off) if ragged else None, min_scores=_i32(torch, mins, np.int32) if ragged else None)
    assert _u64(second) == want
    if name == "edges":
        label = cases.edge_list()[2]
        has = {k: want[r] != 0 for k, r in label.items()}
        assert not (has["above-1"] or has["above+0"] or has["below-1"] or has["below+0"] or has["clamp_in"] or has["copies"] or has["thresh_eq"]
                    or has["best_below"] or has["odd151_in"])
        assert has["above+1"] and has["below+1"] and has["other_strand"] and has["clamp_out"] and has["thresh_above"] and has["odd151_out"]
        assert has["odd149"] == ragged and has["short1"] == ragged                     # dist = len / 2 of the read itself
        assert sel.unpack(want[label["several"]])[:2] == (-19, 10_000 + 5_000 * label["several"] + 2000)
    if name == "random":
        refused = sum(1 for c in cands if c[1] > WORST and sel.selection_key(*c) != best[c[0] >> 34] and want[c[0] >> 34] != sel.selection_key(*c))
        assert refused > 100 and sum(1 for w in want if w) > 100


# ---- mapping quality --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match", [0, 2], ids=["end-to-end", "local"])
@pytest.mark.parametrize("Mr", [50, 150])
def test_mapq_over_a_reads_whole_score_range(amd, orc, Mr, match):
    """every best in [min_score - 1, perfect], every second in [min_score - 1, best] and none, versions 2 and 3, uniform and ragged calls"""
    import torch
    perfect = match * Mr
    min_score = cases.min_score_of(Mr) if match == 0 else int(np.float32(10.0) * np.float32(np.log(np.float32(Mr))))
    pairs = [(b, s) for b in range(min_score - 1, perfect + 1) for s in [None] + list(range(min_score - 1, b + 1))]
    assert len(pairs) > 500
    best = [((b + sel.SCORE_BIAS) << 34) | ((i & 1) << 33) | (1000 + i) for i, (b, _) in enumerate(pairs)]
    second = [0 if s is None else ((s + sel.SCORE_BIAS) << 34) | (5000 + i) for i, (_, s) in enumerate(pairs)]
    off = np.arange(len(pairs) + 1, dtype=np.uint32) * Mr
    mins = np.full(len(pairs), min_score, dtype=np.int32)
    bt, st = _i64(torch, best), _i64(torch, second)
    for version in (2, 3):
        want = sel.mapq_per_read(orc, best, second, version, match == 0, perfect, min_score)
        assert want == sel.mapq_per_read(orc, best, second, version, read_offsets=off, min_scores=mins, match=match)
        q, ss = amd.mapq(bt, st, perfect, min_score, match == 0, version)
        assert _ints(q) == [w[0] for w in want] and _ints(ss) == [w[1] for w in want]
        q, ss = amd.mapq(bt, st, None, None, None, version, read_offsets=_i32(torch, off), min_scores=_i32(torch, mins, np.int32), match=match)
        assert _ints(q) == [w[0] for w in want] and _ints(ss) == [w[1] for w in want]
        q, ss = amd.mapq(bt, None, perfect, min_score, match == 0, version)           # no second alignments at all
        none = sel.mapq_per_read(orc, best, [0] * len(best), version, match == 0, perfect, min_score)
        assert _ints(q) == [w[0] for w in none] and _ints(ss) == [sel.SCORE_MIN] * len(best)
        assert len({w[0] for w in want}) > 10 and want[0][0] == 0     # (a best below min_score maps to 0)


# ---- finish_reads -----------------------------------------------------------------------------------------------------------------
_FINISHED = {}


def _finished(orc, name, cands, n_reads, lengths, ragged, version):
    key = (name, ragged, version)
    if key not in _FINISHED:
        off, mins = cases.ragged_of(lengths)
        _FINISHED[key] = sel.finish_reads(orc, cands, n_reads, DIST, WORST, version, True, 0, MIN_SCORE, read_offsets=off if ragged else None,
                                          min_scores=mins if ragged else None, match=0)
    return _FINISHED[key]


def _check_finish(amd, orc, torch, name, cands, n_reads, lengths, rpt, ragged, version):
    want = _finished(orc, name, cands, n_reads, lengths, ragged, version)
    ordered, toffs = cases.tile_order(cands, rpt, n_reads)
    off, mins = cases.ragged_of(lengths)
    got = amd.finish_reads(*_device(torch, ordered), torch.from_numpy(toffs).cuda(), rpt, n_reads, DIST, WORST, 0, MIN_SCORE, True, version,
                           read_offsets=_i32(torch, off) if ragged else None, min_scores=_i32(torch, mins, np.int32) if ragged else None, match=0)
    assert _u64(got["best"]) == want["best"] and _u64(got["second"]) == want["second"]
    for k in ("best_score", "best_pos", "best_rc", "mapq", "second_score"):
        assert _ints(got[k]) == want[k], k
    return toffs


@pytest.mark.parametrize("rpt", [1, 7, 64, 192])
@pytest.mark.parametrize("name", ["runs", "runs-permuted", "edges", "random"])
def test_finish_reads_against_the_restatement(amd, orc, name, rpt):
    import torch
    cands, n_reads, lengths, _ = _list(name)
    for ragged in ((False, True) if name in ("edges", "random") else (False,)):
        toffs = _check_finish(amd, orc, torch, name, cands, n_reads, lengths, rpt, ragged, 2)
    assert len(toffs) == (n_reads + rpt - 1) // rpt + 1 and toffs[-1] == len(cands)
    if name == "runs":
        assert (np.diff(toffs) == 0).any() or rpt > 1                 # tiles without a candidate (reads_per_tile 1: the empty reads)
        assert np.diff(toffs[::192 // rpt]).max() > 1000              # a workgroup's span far beyond what it keeps in registers


@pytest.mark.parametrize("rpt", [1, 7, 64, 192])
def test_finish_reads_at_the_kept_rounds_boundary(amd, orc, rpt):
    """workgroups whose spans hold exactly 256, 512 and 513 candidates (two rounds of 256 stay in registers, the 513th is loaded again), an empty
    workgroup, and a last tile with one read"""
    import torch
    cands, n_reads = cases.span_list(rpt)
    lengths = [M] * n_reads
    for version in (2, 3):
        toffs = _check_finish(amd, orc, torch, "spans%d" % rpt, cands, n_reads, lengths, rpt, False, version)
    tpg = 192 // rpt
    assert [int(v) for v in np.diff(toffs[::tpg])[:len(cases.SPANS)]] == list(cases.SPANS)
    assert n_reads % rpt == 1 % rpt and toffs[-1] - toffs[-2] == 3 and (np.diff(toffs) == 0).sum() >= tpg
    want = _FINISHED[("spans%d" % rpt, False, 2)]
    assert sum(1 for s in want["second"] if s) > 100 and sum(1 for b in want["best"] if b == 0) > 100


def test_finish_reads_refuses_193_reads_per_tile(amd):
    import torch
    cands, n_reads = cases.random_list(21)
    ordered, toffs = cases.tile_order(cands, 193, n_reads)
    with pytest.raises(amd.NvbioError, match="reads_per_tile"):
        amd.finish_reads(*_device(torch, ordered), torch.from_numpy(toffs).cuda(), 193, n_reads, DIST, WORST, 0, MIN_SCORE, True, 2)


# ---- best windows and the traceback batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "random", "runs-permuted"])
def test_best_windows_and_traceback_batch(amd, name):
    import torch
    cands, n_reads, lengths, best = _list(name)
    G = U32
    want_wb, want_g = sel.best_windows(cands, best)
    keys, scores, sinks, wb = _device(torch, cands)
    bt = _i64(torch, best)
    best_wb = torch.full((n_reads,), -1, dtype=torch.int64, device="cuda")
    best_g = torch.full((n_reads,), -1, dtype=torch.int64, device="cuda")
    amd.best_candidate_windows(keys, scores, sinks, wb, bt, best_wb, best_g)
    assert _ints(best_wb) == want_wb and _ints(best_g) == want_g
    only_wb = torch.full((n_reads,), -1, dtype=torch.int64, device="cuda")
    amd.best_candidate_windows(keys, scores, sinks, wb, bt, only_wb)                   # the locus is optional
    assert _ints(only_wb) == want_wb
    off, mins = cases.ragged_of(lengths)
    for ragged in (False, True):
        want = sel.traceback_batch(best, want_wb, M, BAND, G, MIN_SCORE, read_offsets=off if ragged else None, min_scores=mins if ragged else None)
        flags, jb, je, js, jk = amd.traceback_best_batch(bt, best_wb, M, BAND, G, MIN_SCORE, read_offsets=_i32(torch, off) if ragged else None,
                                                         min_scores=_i32(torch, mins, np.int32) if ragged else None)
        assert _ints(flags) == [w[0] for w in want]
        assert _u32s(amd, jb) == [w[1] for w in want] and _u32s(amd, je) == [w[2] for w in want]
        assert _ints(js) == [w[3] for w in want]
        assert [tuple(int(v) for v in row) for row in amd.u32(jk)] == [w[4] for w in want]
        if name == "edges":
            label = cases.edge_list()[2]
            p = lambda k: 10_000 + 5_000 * label[k]
            assert want_wb[label["tie_whole_key"]] == p("tie_whole_key") - 145 and want[label["tie_whole_key"]][4][0] == 145     # the largest window begin of three
            assert want_g[label["locus0"]] == 0 and want_wb[label["locus0"]] == 0
            assert want[label["end_clamped"]][1:3] == (U32 - 100, G) and want[label["field33"]][2] == G
            for k in ("empty", "best_below", "rej_alone", "m20+1"):
                assert want[label[k]] == sel.EMPTY_JOB, k
            assert want_wb[label["empty"]] == -1 and want_wb[label["best_below"]] >= 0
            assert want[label["short1"]][4][1] == (1 if ragged else M)


# ---- opposite-mate windows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1_000_000, U32], ids=["1M", "4G"])
def test_opposite_mate_windows(amd, G):
    import torch
    gs = [0, 1, 99, 100, 101, 499, 500, 501, 5000, G - 1, G - 100, G - 501] + ([U32 - 300, U32 - 2] if G == U32 else [G, G + 7])
    g_pos = _i32(torch, gs + gs)
    rcs = [0] * len(gs) + [1] * len(gs)
    rc_t = torch.tensor(rcs, dtype=torch.uint8, device="cuda")
    valid = invalid = wrapped = 0
    # (anchor_len, opposite_gapped_len, min_frag, max_frag): the default, max_frag < anchor_len, a narrow range, min_frag > g + a_len + o_len, tiny mates
    frames = ((100, 110, 0, 500), (100, 110, 0, 50), (100, 110, 400, 500), (150, 160, 2000, 3000), (1, 1, 0, 1))
    for policy, anchor, overlap, (a_len, o_len, lo, hi) in itertools.product(range(4), (0, 1), (False, True), frames):
        want = [sel.opposite_window(g, rc, a_len, o_len, anchor, policy, lo, hi, overlap, G) for g, rc in zip(gs + gs, rcs)]
        wb, we, flags, ok = amd.opposite_mate_windows(g_pos, rc_t, a_len, o_len, anchor, G, policy=policy, min_frag_len=lo, max_frag_len=hi, overlap=overlap)
        assert _u32s(amd, wb) == [w[0] for w in want] and _u32s(amd, we) == [w[1] for w in want]
        assert _ints(flags) == [w[2] for w in want] and _ints(ok) == [w[3] for w in want]
        valid += sum(w[3] for w in want)
        invalid += sum(1 for w in want if not w[3])
        assert all(w[:2] == (0, 0) for w in want if not w[3])
        wrapped += sum(1 for g, w in zip(gs + gs, want) if g + hi >= 1 << 32 and w[3])
    assert valid > 500 and invalid > 500 and (wrapped > 0) == (G == U32)


# ---- the score stream -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [500_000, U32], ids=["500k", "4G"])
@pytest.mark.parametrize("band", [0, 1, 31, 32])
def test_score_stream_at_its_edges(amd, band, G):
    """loci that wrapped below zero, windows whose end wraps uint32 or that begin past the genome, a NULL and a permuted idx_queue, the worst clamp"""
    import torch
    rng = np.random.default_rng(band + 50)
    read_index, rid, seed, loc = cases.edge_stream(G, band)
    H = len(rid)
    empties = 0
    for q in (None, rng.permutation(H)[:H - 9].astype(np.uint32)):
        for rev in (True, False):
            hq = amd.HitQueues(rid, seed, loc, idx_queue=q)
            want = sel.stream_flatten(q, rid, seed, loc, read_index, band, G, rev)
            got = amd.score_stream_flatten(hq, read_index, band, G, rev)
            assert _u32s(amd, got[0]) == [w[0] for w in want] and _ints(got[1]) == [w[1] for w in want]
            assert _u32s(amd, got[2]) == [w[2] for w in want] and _u32s(amd, got[3]) == [w[3] for w in want]
        n = len(want)
        empties += sum(1 for w in want if w[2:] == (0, 0))
        scores = rng.integers(-70000, 10, n).astype(np.int32)
        scores[:3] = (-65537, -65536, -65535)
        sinks = np.stack([rng.integers(0, 200, n), rng.integers(0, 160, n)], axis=1).astype(np.uint32)
        wbn = np.array([w[2] for w in want], dtype=np.uint32)
        amd.score_stream_output(hq, torch.from_numpy(scores).cuda(), torch.from_numpy(sinks.view(np.int32)).cuda(), got[2])
        out = sel.stream_output(q, H, scores, sinks[:, 0], wbn, -65536)
        hs, hk = _ints(hq.score), _u32s(amd, hq.sink)
        assert all((hs[h], hk[h]) == out[h] for h in out) and len(out) == n
        assert all(hs[h] == 0 and hk[h] == 0 for h in range(H) if h not in out)          # hits outside the queue are not written
        assert min(v[0] for v in out.values()) == -65536
    assert empties >= 8


# ---- the sw-benchmark conversions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_text_le_to_be_and_scores_to_int16(amd, n):
    import torch
    rng = np.random.default_rng(n)
    words = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for i in range(n):                                                # word i: symbol (i + n) / 16 % 4 at slot (i + n) % 16, so every symbol meets every slot
        slot, sym = (i + n) % 16, ((i + n) // 16) % 4
        words[i] = (int(words[i]) & ~(3 << (2 * slot)) & U32) | (sym << (2 * slot))
    got = amd.text_2bit_le_to_be(torch.from_numpy(words.view(np.int32)).cuda())
    assert _u32s(amd, got) == [sel.le_to_be_word(int(w)) for w in words]
    if n >= 255:
        assert {((i + n) % 16, ((i + n) // 16) % 4) for i in range(n)} >= set(itertools.product(range(16), range(4)))
    scores = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    edge = [32767, 32768, -32768, -32769, sel.SCORE_MIN]
    scores[:min(n, 5)] = edge[:min(n, 5)]
    if n > 5:
        scores[-5:] = edge
    got = amd.scores_to_int16(torch.from_numpy(scores).cuda())
    assert got.dtype == torch.int16 and _ints(got) == [sel.to_int16(int(v)) for v in scores]
