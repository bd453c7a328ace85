"""The candidate lists the selection-stage tests share (test_selection_oracle.py pins the restatement on them, test_gpu_selection_edges.py
runs the kernels on them): built once, never modified.  A candidate is (key, score, win_begin, sink_x), see selection_cpu.py."""
import functools

import numpy as np

import selection_cpu as sel

M = 150                                   # read length of the uniform calls
DIST = M // 2
MIN_SCORE = -90                           # end-to-end: int(-0.6 - 0.6 * 150)
WORST = MIN_SCORE - 1
BAND = 31
U32 = 0xFFFFFFFF
RUN_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 256, 257, 1000)
RUN_LANES = (0, 1, 63)
SPANS = (256, 512, 513, 0, 700)           # candidates per workgroup of finish_reads: around its FINISH_KEPT = 2 rounds of 256, and an empty one


def cand(rid, strand, score, pos, sink_x=160, field=None):
    """a candidate of read rid ending at pos (= win_begin + sink_x); its diagonal field defaults to the window's middle"""
    wb = pos - sink_x
    assert 0 <= wb <= U32
    return ((rid << 34) | (strand << 33) | (wb + BAND // 2 + sel.BIAS if field is None else field), score, wb, sink_x)


def min_score_of(length):
    return int(np.float32(-0.6) + np.float32(-0.6) * np.float32(length))


@functools.lru_cache(maxsize=None)
def run_list():
    """runs of RUN_LENGTHS candidates of one read, each starting at lane 0, 1 and 63 of a wave, the maximum at the run's first, a middle and
    its last candidate; a read without candidates before every run; single-candidate reads fill up to the lane
    -> (cands, n_reads, runs = [(read, first index, length, index of the maximum)])"""
    rng = np.random.default_rng(4100)
    cands, runs, rid = [], [], 0
    for n in RUN_LENGTHS:
        for lane in RUN_LANES:
            for where in (0, n // 2, n - 1):
                while len(cands) % 64 != lane:
                    cands.append(cand(rid, int(rng.integers(0, 2)), int(rng.integers(-80, -9)), int(rng.integers(1000, 1 << 32))))
                    rid += 1
                rid += 1                                              # a read without candidates
                first = len(cands)
                for j in range(n):
                    score = 0 if j == where else int(rng.integers(-80, -9))
                    cands.append(cand(rid, int(rng.integers(0, 2)), score, int(rng.integers(1000, 1 << 32))))
                runs.append((rid, first, n, first + where))
                rid += 1
    return tuple(cands), rid + 1, tuple(runs)                         # (the last read has no candidate either)


@functools.lru_cache(maxsize=None)
def permuted_run_list():
    cands, n_reads, _ = run_list()
    order = np.random.default_rng(4101).permutation(len(cands))
    return tuple(cands[i] for i in order), n_reads


@functools.lru_cache(maxsize=None)
def edge_list():
    """one read per edge -> (cands, n_reads, label -> read, read lengths for the ragged calls)"""
    reads, label = [], {}

    def P(r):
        return 10_000 + 5_000 * r

    def add(name, make, length=M):
        r = len(reads)
        label[name] = r
        reads.append((make(r, P(r)), length))

    add("empty", lambda r, p: [])
    add("tie", lambda r, p: [cand(r, 0, -20, p + 4000), cand(r, 1, -20, p + 100), cand(r, 1, -20, p + 200)])          # strand, then position
    add("field33", lambda r, p: [cand(r, 0, -10, 0xFFFFFFF0 + 200, 200), cand(r, 1, -30, p)])                         # end position >= 2^32
    for name, s in (("m20-1", -(1 << 20) - 1), ("m20", -(1 << 20)), ("m20+1", -(1 << 20) + 1)):
        add(name, lambda r, p, s=s: [cand(r, 0, s, p)])
    add("m20all", lambda r, p: [cand(r, 0, -(1 << 20) - 1, p + 900), cand(r, 1, -(1 << 20), p + 600), cand(r, 0, -(1 << 20) + 1, p)])
    add("rej_alone", lambda r, p: [cand(r, 1, sel.SCORE_MIN, p + U32, U32)])
    add("rej_two", lambda r, p: [cand(r, 0, sel.SCORE_MIN, p + 7 + U32, U32), cand(r, 1, sel.SCORE_MIN, p + U32, U32)])
    add("rej_beside", lambda r, p: [cand(r, 1, sel.SCORE_MIN, p + U32, U32), cand(r, 0, -15, p), cand(r, 0, sel.SCORE_MIN, p + 3 + U32, U32)])
    for d in (DIST - 1, DIST, DIST + 1):
        add("above%+d" % (d - DIST), lambda r, p, d=d: [cand(r, 0, -5, p), cand(r, 0, -20, p + d)])
        add("below%+d" % (d - DIST), lambda r, p, d=d: [cand(r, 1, -20, p - d), cand(r, 1, -5, p)])
    add("other_strand", lambda r, p: [cand(r, 0, -5, p), cand(r, 1, -20, p)])
    add("clamp_in", lambda r, p: [cand(r, 0, -5, 100, 100), cand(r, 0, -20, 30, 30)])           # pos2 < dist: the lower bound clamps at 0
    add("clamp_out", lambda r, p: [cand(r, 0, -5, 100, 100), cand(r, 0, -20, 20, 20)])          # ... and 100 > 20 + 75
    add("copies", lambda r, p: [cand(r, 0, -5, p)] * 3 + [cand(r, 0, -30, p + 10)])
    add("thresh_eq", lambda r, p: [cand(r, 0, -5, p), cand(r, 1, WORST, p)])
    add("thresh_above", lambda r, p: [cand(r, 0, -5, p), cand(r, 1, WORST + 1, p)])
    add("best_below", lambda r, p: [cand(r, 0, -100, p), cand(r, 1, -95, p + 1000)])
    add("several", lambda r, p: [cand(r, 0, -5, p), cand(r, 0, -20, p + 1000), cand(r, 1, -20, p + 50), cand(r, 0, -19, p + 2000), cand(r, 1, -40, p + 5),
                                 cand(r, 0, -19, p + 1900)])
    add("odd151_in", lambda r, p: [cand(r, 0, -5, p), cand(r, 0, -20, p + 75)], 151)
    add("odd151_out", lambda r, p: [cand(r, 0, -5, p), cand(r, 0, -20, p + 76)], 151)
    add("odd149", lambda r, p: [cand(r, 0, -5, p), cand(r, 0, -20, p + 75)], 149)              # distinct at dist 74, not at 75
    add("short1", lambda r, p: [cand(r, 1, 0, p, 1), cand(r, 1, 0, p + 1, 1)], 1)               # dist 0: one position apart is distinct
    add("tie_whole_key", lambda r, p: [cand(r, 0, -10, p, 150), cand(r, 0, -10, p, 160), cand(r, 0, -10, p, 145), cand(r, 1, -11, p, 100)])
    add("locus0", lambda r, p: [cand(r, 0, -10, 120, 120, field=1000)])                          # a diagonal below the genome start
    add("end_clamped", lambda r, p: [cand(r, 1, -10, U32 - 100 + 160, 160)])                     # win_begin + band + M > 0xFFFFFFFF
    add("last", lambda r, p: [cand(r, 0, -1, p)])
    cands = [c for cs, _ in reads for c in cs]
    return tuple(cands), len(reads), dict(label), tuple(l for _, l in reads)


def ragged_of(lengths):
    """(read_offsets uint32 [R + 1], min_scores int32 [R]) of reads of the given lengths"""
    off = np.zeros(len(lengths) + 1, dtype=np.uint32)
    off[1:] = np.cumsum(lengths)
    return off, np.array([min_score_of(l) for l in lengths], dtype=np.int32)


def random_list(seed, n_reads=300, n=3000):
    """candidates of random reads, close enough together that many are not distinct; in read order"""
    rng = np.random.default_rng(seed)
    base = rng.integers(1000, 1 << 31, n_reads)
    rid = np.sort(rng.integers(0, n_reads, n))
    return tuple(cand(int(r), int(rng.integers(0, 2)), int(rng.integers(-110, 1)), int(base[r]) + int(rng.integers(0, 300)), int(rng.integers(140, 181)))
                 for r in rid), n_reads


def reads_per_group(rpt):
    return (192 // rpt) * rpt


@functools.lru_cache(maxsize=None)
def span_list(rpt):
    """tile-ordered candidates for finish_reads at reads_per_tile = rpt: workgroup w (192 // rpt tiles) holds exactly SPANS[w] candidates, spread
    over its reads in any order; then one last tile with a single read -> (cands, n_reads)"""
    rng = np.random.default_rng(4200 + rpt)
    rpg = reads_per_group(rpt)
    cands = []
    for w, span in enumerate(SPANS):
        base = rng.integers(1000, 1 << 31, rpg)
        group = []
        for _ in range(span):
            r = int(rng.integers(0, rpg))
            group.append(cand(w * rpg + r, int(rng.integers(0, 2)), int(rng.integers(-110, 1)), int(base[r]) + int(rng.integers(0, 300)), int(rng.integers(140, 181))))
        group.sort(key=lambda c: (c[0] >> 34) // rpt)                 # tile order; within a tile as drawn
        cands += group
    last = len(SPANS) * rpg
    cands += [cand(last, 1, -7, 5000), cand(last, 1, -9, 5020), cand(last, 0, -30, 9000)]
    return tuple(cands), last + 1


def tile_order(cands, rpt, n_reads):
    """stable sort by tile -> (cands, tile_offsets int32 [n_tiles + 1])"""
    n_tiles = (n_reads + rpt - 1) // rpt
    out = sorted(cands, key=lambda c: (c[0] >> 34) // rpt)
    counts = np.bincount([(c[0] >> 34) // rpt for c in out], minlength=n_tiles)
    return out, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


BIG_N = (1 << 21) + 321                   # one more candidate than 8192 blocks of 256 threads take in one stride, and 320 more


@functools.lru_cache(maxsize=None)
def big_list():
    """BIG_N candidates in read order as arrays (keys uint64, scores int32, win_begin uint32, sink_x uint32), n_reads"""
    rng = np.random.default_rng(4300)
    n_reads = 4001
    rid = np.sort(rng.integers(0, n_reads - 1, BIG_N)).astype(np.uint64)     # (the last read keeps no candidate)
    strand = rng.integers(0, 2, BIG_N).astype(np.uint64)
    wb = rng.integers(0, 1 << 32, BIG_N, dtype=np.uint64).astype(np.uint32)
    keys = (rid << np.uint64(34)) | (strand << np.uint64(33)) | (wb.astype(np.uint64) + np.uint64(BAND // 2 + sel.BIAS))
    scores = rng.integers(-300, 1, BIG_N).astype(np.int32)
    sink_x = rng.integers(100, 200, BIG_N).astype(np.uint32)
    return keys, scores, wb, sink_x, n_reads


# ---- keys and windows -------------------------------------------------------------------------------------------------------------
def key_hits(seeds_per_read, seed_interval, seed_len, read_len, n_ids):
    """(text_pos, seed_id) pairs: every seed id below n_ids at text positions 0, 1, 2^32 - 1 - seed_len and p - 1, p, p + 1 for the seed's
    offset p on either strand"""
    hits = []
    for sid in range(n_ids):
        ps = {sel.seed_offset(sid, seeds_per_read, seed_interval, seed_len, read_len, s) for s in (0, 1)}
        pos = {0, 1, U32 - seed_len} | {p + d for p in ps for d in (-1, 0, 1) if p + d >= 0}
        hits += [(t, sid) for t in sorted(pos)]
    return hits


def window_keys(band, read_len, genome_len, n_reads):
    """diagonal keys whose windows sit on every edge of the rule for this band: the genome start, the clamp of the diagonal, the half band,
    the genome end exactly and one past it; both strands, reads cycling"""
    half = band // 2
    fields = [0, 1023, 1024, 1025, 1024 + half - 1, 1024 + half, 1024 + half + 1]
    for over in (-1, 0, 1, 2):                                        # begin + band + read_len = genome_len + over
        begin = genome_len + over - band - read_len
        fields.append(begin + half + sel.BIAS)
    fields += [genome_len - 1 + sel.BIAS, genome_len + sel.BIAS - half - 1]
    fields = [f for f in fields if 0 <= f <= U32 + sel.BIAS]         # (a diagonal is a text position below 2^32 minus a seed offset)
    return [((i % n_reads) << 34) | ((i & 1) << 33) | f for i, f in enumerate(fields + fields)]


# ---- the scoring stream -----------------------------------------------------------------------------------------------------------
def edge_stream(genome_len, band):
    """hit queues whose loci sit on the stream's edges -> (read_index, hit_read_id, hit_seed, hit_loc)"""
    lens = [30, 1, 159, 100]
    read_index = np.zeros(len(lens) + 1, dtype=np.uint32)
    read_index[1:] = np.cumsum(lens)
    loc = [0, 1, band // 2, band // 2 + 1, 0xFFFFFFF0, U32, genome_len - 1, genome_len, genome_len + band // 2, genome_len + band // 2 + 1,
           genome_len - 100, U32 - 40, U32 - band - 30 + band // 2, 5000]
    loc = [l & U32 for l in loc]
    H = len(loc) * len(lens) * 2
    hit_loc = np.array([loc[h % len(loc)] for h in range(H)], dtype=np.uint32)
    hit_read_id = np.array([(h // len(loc)) % len(lens) for h in range(H)], dtype=np.uint32)
    rc = np.array([h // (len(loc) * len(lens)) for h in range(H)], dtype=np.uint32)
    hit_seed = ((np.arange(H, dtype=np.uint32) * 37) & 0xFFF) | (rc << 13) | (np.uint32(1) << 14)
    return read_index, hit_read_id, hit_seed.astype(np.uint32), hit_loc
