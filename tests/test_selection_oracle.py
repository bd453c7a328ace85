"""CPU: the restatement of the selection stage (selection_cpu.py) pinned to what the oracle already holds -- nvBowtie's score_reduce loop,
the opposite-mate window, the scoring stream -- on random lists and on the edge lists the GPU tests run (selection_cases.py), plus keys and
windows computed by hand, and the diagonal-key underflow shown in plain integers."""
import itertools

import numpy as np
import pytest

from oracle import cpu_pipeline

import selection_cases as cases
import selection_cpu as sel

U32 = 0xFFFFFFFF


def _by_read(cands, n_reads):
    per = [[] for _ in range(n_reads)]
    for c in cands:
        per[c[0] >> 34].append(c)
    return per


def _pin_to_score_reduce(orc, cands, n_reads, lengths):
    """best and second best of every read against the oracle's score_reduce loop fed in descending key order (reads whose positions fit
    uint32 with room for + dist, and whose scores the key does not clamp) -> how many reads were compared, how many had a second"""
    off, mins = cases.ragged_of(lengths)
    best = sel.best_per_read(cands, n_reads)
    second = sel.second_per_read(cands, best, None, None, read_offsets=off, min_scores=mins)
    compared = seconds = 0
    for r, cs in enumerate(_by_read(cands, n_reads)):
        keys = sorted((sel.selection_key(*c) for c in cs), reverse=True)
        if not cs or any((k & sel.FIELD) + lengths[r] >= 1 << 32 for k in keys) or any(c[1] <= -(1 << 20) for c in cs):
            continue
        un = [sel.unpack(k) for k in keys]
        worst = int(mins[r]) - 1
        a1, s1, p1, rc1, a2, s2, p2, rc2 = orc.score_reduce([u[0] for u in un], [u[1] for u in un], [u[2] for u in un], lengths[r], worst)
        if a1:
            assert (s1, p1, rc1) == sel.unpack(best[r]), r
        else:
            assert sel.unpack(best[r])[0] <= worst and second[r] == 0, r
        assert bool(a2) == (second[r] != 0), r
        if a2:
            assert (s2, p2, rc2) == sel.unpack(second[r]), r
            seconds += 1
        compared += 1
    return compared, seconds


def _refused_as_not_distinct(cands, best, dist, worst):
    """candidates above the threshold that are not the best and lose only to the distinctness rule"""
    n = 0
    for c in cands:
        s, b = sel.selection_key(*c), best[c[0] >> 34]
        n += c[1] > worst and s != b and not sel.distinct(b & sel.FIELD, (b >> 33) & 1, s & sel.FIELD, (s >> 33) & 1, dist)
    return n


def test_best_and_second_equal_score_reduce_on_the_edge_list(orc):
    cands, n_reads, label, lengths = cases.edge_list()
    compared, seconds = _pin_to_score_reduce(orc, cands, n_reads, lengths)
    assert compared >= n_reads - 10 and seconds >= 8
    # what the list was built for, in the restatement's own terms (uniform calls: dist 75, threshold -91)
    best = sel.best_per_read(cands, n_reads)
    second = sel.second_per_read(cands, best, cases.DIST, cases.WORST)
    got = {name: second[r] != 0 for name, r in label.items()}
    for name in ("above-1", "above+0", "below-1", "below+0", "clamp_in", "copies", "thresh_eq", "best_below", "odd151_in", "odd149", "short1", "empty"):
        assert not got[name], name
    for name in ("above+1", "below+1", "other_strand", "clamp_out", "thresh_above", "several", "odd151_out", "tie"):
        assert got[name], name
    assert sel.unpack(best[label["tie"]])[1:] == (10_000 + 5_000 * label["tie"] + 200, 1)
    assert sel.unpack(second[label["several"]])[:2] == (-19, 10_000 + 5_000 * label["several"] + 2000)
    assert sel.unpack(best[label["field33"]])[1] >= 1 << 32
    off, mins = cases.ragged_of(lengths)
    ragged = sel.second_per_read(cands, best, None, None, read_offsets=off, min_scores=mins)
    assert ragged[label["odd149"]] != 0 and ragged[label["short1"]] != 0 and ragged[label["odd151_in"]] == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_best_and_second_equal_score_reduce_on_random_lists(orc, seed):
    cands, n_reads = cases.random_list(seed)
    compared, seconds = _pin_to_score_reduce(orc, cands, n_reads, [cases.M] * n_reads)
    assert compared > 200 and seconds > 50
    best = sel.best_per_read(cands, n_reads)
    assert _refused_as_not_distinct(cands, best, cases.DIST, cases.WORST) > 100


def test_the_run_list_is_what_it_claims():
    cands, n_reads, runs = cases.run_list()
    best = sel.best_per_read(cands, n_reads)
    assert {(n, first % 64) for _, first, n, _ in runs} == set(itertools.product(cases.RUN_LENGTHS, cases.RUN_LANES))
    assert sum(1 for _, first, n, _ in runs if first % 64 + n > 64) >= 60         # runs that straddle a wave
    for rid, first, n, top in runs:
        assert best[rid] == sel.selection_key(*cands[top]) and best[rid - 1] == 0
        assert all(c[0] >> 34 == rid for c in cands[first:first + n])
    assert sel.best_per_read(cases.permuted_run_list()[0], n_reads) == best


def test_unpack_of_a_rejected_only_read_and_the_clamp_at_minus_2_20():
    cands, n_reads, label, _ = cases.edge_list()
    best = sel.best_per_read(cands, n_reads)
    p = 10_000 + 5_000 * label["rej_alone"]
    assert best[label["rej_alone"]] == (1 << 33) | (p + U32) and sel.unpack(best[label["rej_alone"]]) == (sel.SCORE_MIN, p + U32, 1)
    assert sel.unpack(best[label["rej_two"]])[0] == sel.SCORE_MIN and sel.unpack(best[label["rej_two"]])[2] == 1
    assert sel.unpack(best[label["rej_beside"]]) == (-15, 10_000 + 5_000 * label["rej_beside"], 0)
    assert sel.unpack(best[label["m20-1"]])[0] == sel.SCORE_MIN and sel.unpack(best[label["m20"]])[0] == sel.SCORE_MIN
    assert sel.unpack(best[label["m20+1"]])[0] == -(1 << 20) + 1 and sel.unpack(best[label["m20all"]])[0] == -(1 << 20) + 1
    assert sel.unpack(0) == (sel.SCORE_MIN, -1, 0)


def test_numpy_twins_equal_the_plain_functions():
    for cands, n_reads in (cases.random_list(5), cases.edge_list()[:2], cases.run_list()[:2]):
        keys = np.array([c[0] for c in cands], dtype=np.uint64)
        scores = np.array([c[1] for c in cands], dtype=np.int32)
        wb = np.array([c[2] for c in cands], dtype=np.uint32)
        sx = np.array([c[3] for c in cands], dtype=np.uint32)
        s = sel.selection_keys_np(keys, scores, wb, sx)
        assert [int(v) for v in s] == sel.selection_keys(cands)
        best = sel.best_per_read_np(keys, s, n_reads)
        assert [int(v) for v in best] == sel.best_per_read(cands, n_reads)
        sc, pos, rc = sel.unpack_np(best)
        assert [(int(a), int(b), int(c)) for a, b, c in zip(sc, pos, rc)] == [sel.unpack(int(b)) for b in best]


def test_opposite_window_equals_the_oracle_over_all_policies():
    valid = invalid = 0
    for G in (1_000_000, U32):
        gs = [0, 1, 99, 100, 101, 499, 500, 501, 5000, G - 1, G - 100, G - 501] + ([U32 - 300, U32 - 1] if G == U32 else [G, G + 7])
        for policy, anchor, rc, overlap, g in itertools.product(range(4), (0, 1), (0, 1), (False, True), gs):
            for a_len, o_len, lo, hi in ((100, 110, 0, 500), (100, 110, 0, 50), (100, 110, 400, 500), (150, 160, 2000, 3000), (1, 1, 0, 1)):
                got = sel.opposite_window(g, rc, a_len, o_len, anchor, policy, lo, hi, overlap, G)
                b, e, fw, ok = cpu_pipeline.opposite_window(g, not rc, a_len, o_len, anchor, G, policy=policy, min_frag=lo, max_frag=hi, overlap=overlap)
                assert got[3] == (1 if ok else 0) and got[2] == (0 if fw else 3)
                assert got[:2] == ((b, e) if ok else (0, 0))
                valid += got[3]
                invalid += 1 - got[3]
    assert valid > 1000 and invalid > 1000


@pytest.mark.parametrize("G", [500_000, U32])
@pytest.mark.parametrize("band", [0, 1, 31, 32])
def test_stream_flatten_and_output_equal_the_oracle(G, band):
    rng = np.random.default_rng(band + 11)
    read_index, rid, seed, loc = cases.edge_stream(G, band)
    H = len(rid)
    for q in (None, rng.permutation(H)[:H - 9].astype(np.uint32)):
        for rev in (True, False):
            got = sel.stream_flatten(q, rid, seed, loc, read_index, band, G, rev)
            want = cpu_pipeline.score_stream_flatten(q, rid, seed, loc, read_index, band, G, rev)
            assert got == [tuple(int(w[i]) for w in want) for i in range(len(got))]
        n = len(got)
        scores = rng.integers(-70000, 10, n).astype(np.int32)
        sinks = np.stack([rng.integers(0, 200, n), rng.integers(0, 160, n)], axis=1).astype(np.uint32)
        wb = np.array([g[2] for g in got], dtype=np.uint32)
        out = sel.stream_output(q, H, scores, sinks[:, 0], wb, -65536)
        ws, wk = cpu_pipeline.score_stream_output(q, H, scores, sinks, wb)
        assert all(out[h] == (int(ws[h]), int(wk[h])) for h in out) and len(out) == n
    assert sum(1 for g in got if g[2:] == (0, 0)) >= 4 and (scores < -65536).any()


def test_keys_and_windows_by_hand():
    # seeds_per_read 13, interval 10, seed length 22, read length 150: seed id 27 = read 2, seed 1: offset 10 forward, 150 - 10 - 22 = 118 reverse
    assert sel.hit_to_diagonal(5000, 27, 13, 10, 22, 150, 0) == (2 << 34) | (5000 - 10 + 1024)
    assert sel.hit_to_diagonal(5000, 27, 13, 10, 22, 150, 1) == (2 << 34) | (1 << 33) | (5000 - 118 + 1024)
    assert sel.hit_to_diagonal(0, 12, 13, 10, 22, 150, 0) == 1024 - 120                          # the last seed at the genome start
    assert sel.hit_to_diagonal(0, 0, 13, 10, 22, 150, 1) == (1 << 33) | (1024 - 128)
    assert sel.hit_to_diagonal(U32 - 22, 13, 13, 10, 22, 150, 0) == (1 << 34) | (U32 - 22 + 1024)
    assert sel.hit_to_diagonal(0, 1, 2, 1024, 22, 1046, 0) == 0                                  # read_len - seed_len = 1024: the field's floor
    # (key, band, read length, genome length) -> (read, flags, begin, end)
    assert sel.window((7 << 34) | 6024, 31, 150, 1 << 30) == (7, 0, 4985, 5166)
    assert sel.window((7 << 34) | (1 << 33) | 6024, 31, 150, 1 << 30) == (7, 3, 4985, 5166)
    assert sel.window(1000, 31, 150, 1 << 30) == (0, 0, 0, 181)                                  # diagonal -24
    assert sel.window(1024 + 15, 31, 150, 1 << 30) == (0, 0, 0, 181)                             # g = band / 2: not above it
    assert sel.window(1024 + 16, 31, 150, 1 << 30) == (0, 0, 1, 182)
    assert sel.window(1024 + 16, 32, 150, 1 << 30) == (0, 0, 0, 182)
    assert sel.window(1024 + 5000, 0, 150, 5150) == (0, 0, 5000, 5150)                           # the end exactly at the genome's
    assert sel.window(1024 + 5000, 0, 150, 5149) == (0, 0, 5000, 5149)
    assert sel.window(1024 + U32, 31, 150, U32) == (0, 0, U32 - 15, U32)                         # begin + band + read_len >= 2^32
    assert sel.windows([(1 << 34) | 6024], 30, None, 1 << 30, read_offsets=[0, 100, 1123]) == [(1, 0, 4985, 4985 + 30 + 1023)]
    assert sel.selection_key((3 << 34) | (1 << 33) | 6024, -12, 4985, 160) == ((1 << 20) - 12 << 34) | (1 << 33) | 5145
    assert sel.selection_key(0, sel.SCORE_MIN, 5, U32) == 5 + U32
    assert sel.traceback_job(((1 << 20) - 12 << 34) | (1 << 33) | 5145, 4985, 150, 31, 5100, -90) == (3, 4985, 5100, -12, (160, 150))
    assert sel.traceback_job(((1 << 20) - 12 << 34) | 5145, 4985, 150, 31, 1 << 30, -11) == sel.EMPTY_JOB
    assert sel.le_to_be_word(0x00000003) == 0xC0000000 and sel.le_to_be_word(0x80000001) == 0x40000002
    assert [sel.to_int16(v) for v in (32767, 32768, -32768, -32769, sel.SCORE_MIN)] == [32767, -32768, -32768, 32767, 0]


def test_le_to_be_equals_the_oracles_packing(orc):
    rng = np.random.default_rng(9)
    syms = rng.integers(0, 4, 16 * 40, dtype=np.uint8)
    le = [sum(int(s) << (2 * i) for i, s in enumerate(syms[w * 16:w * 16 + 16])) for w in range(40)]
    assert [sel.le_to_be_word(w) for w in le] == [int(w) for w in orc.pack2(syms)[:40]]


def test_mapq_restatement_calls_the_oracle(orc):
    b, s = ((1 << 20) - 10) << 34 | 777, ((1 << 20) - 40) << 34 | 99
    assert sel.mapq(orc, b, s, 2, True, 0, -90) == (orc.mapq(2, True, 0, -90, -10, True, -40), -40)
    assert sel.mapq(orc, b, 0, 3, False, 300, 50) == (orc.mapq(3, False, 300, 50, -10, False, sel.SCORE_MIN), sel.SCORE_MIN)
    assert sel.mapq(orc, 0, 0, 2, True, 0, -90) == (0, sel.SCORE_MIN)
    assert sel.mapq(orc, (1 << 33) | 5, 0, 2, True, 0, -90)[0] == 0                               # a rejected-only read: best -2^20 < min_score


def test_the_diagonal_key_underflow_in_plain_integers():
    """read_len - seed_len > 1024: a hit of the last seed within (offset - 1024) symbols of the genome start leaves the field below zero;
    formed in 64-bit unsigned arithmetic the key then names read 2^30 - 1.  At the limit the field's floor is 0."""
    spr, interval, L, Mlong = 2, 1100, 22, 1122                        # last seed offset 1100 = read_len - seed_len
    assert sel.diagonal_field(0, sel.seed_offset(1, spr, interval, L, Mlong, 0)) == -76
    assert sel.diagonal_field(75, 1100) == -1 and sel.diagonal_field(76, 1100) == 0
    with pytest.raises(ValueError):
        sel.hit_to_diagonal(0, 1, spr, interval, L, Mlong, 0)
    bad = sel.hit_to_diagonal_wrapped(0, 5 * spr + 1, spr, interval, L, Mlong, 0)
    assert bad >> 34 == (1 << 30) - 1 and (bad >> 33) & 1 == 1        # not read 5, not the forward strand
    assert sel.hit_to_diagonal_wrapped(76, 5 * spr + 1, spr, interval, L, Mlong, 0) == 5 << 34
    # the same on the reverse strand: seed 0 lies at read_len - seed_len
    assert sel.diagonal_field(0, sel.seed_offset(0, spr, interval, L, Mlong, 1)) == -76
    # within the limit no text position leaves the field, on either side
    for p in (0, 1, sel.MAX_SEED_OFFSET):
        assert 0 <= sel.diagonal_field(0, p) and sel.diagonal_field(U32, p) <= sel.FIELD
    assert sel.diagonal_field(0, sel.MAX_SEED_OFFSET + 1) < 0
