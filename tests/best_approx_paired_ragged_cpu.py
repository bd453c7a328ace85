"""Test infrastructure: nvBowtie's PAIRED-END best-approx loop over mates of DIFFERENT lengths, restated pass by pass over the whole batch.  It is
oracle/cpu_pipeline.nvbowtie_best_approx_paired_cpu with every quantity the reference takes from a read's own range made per pair: the anchor's
length M and the opposite mate's Mo (BestAnchorScoreStream / BestOppositeScoreStream, score_inl.h:206-213, :341-347, :398-399), the seed interval S,
the first seed offset of a pass and the filter (map_kernel, mapping_inl.h:504-529), the worst / perfect scores and the distinct distance M / 2 of the
anchor read (score_reduce_paired_kernel, reduce_inl.h:184-185,240,271).  n_multi stays a batch-wide number.

The contract it restates (include/nvbio_amd.h, nvbio_pe_ragged; host/nvbio_amd/best_approx.hpp, best_approx_paired_ragged):
  * per anchor the seeds of the single-end ragged route over the anchor mate's lengths (tests/best_approx_ragged_cpu.py);
  * the filter applies to seeding only: a mate with M < max( min_read_len, seed_len ) has an empty deque in every pass while it is the anchor and is
    never reseeded, but is aligned as the opposite mate of its partner's hits; a pair whose both mates are filtered ends as initialised
    (the reference would seed a mate with min_read_len <= M < seed_len once with the whole read: the library's one divergence);
  * seeding of an anchor stops only when no read of the batch has a seed slot left.
Also here: the ragged pairs the CPU and GPU tests share, and the references over them, computed once per process."""
import numpy as np

from best_approx_ragged_cpu import min_score_e2e, seed_tables, stored_stream  # noqa: F401  (stored_stream: for the GPU tests)
import pe_steps_cpu as pe
from oracle.cpu_pipeline import SCORE_MIN
from util import mutate_reads

FIXED_PAIRS = ((11, 100), (100, 21), (21, 11), (22, 150), (150, 22), (23, 23), (30, 250), (250, 30), (1023, 100), (100, 1023))
N_PAIRS, N_REPEAT, N_ELSEWHERE, N_RANDOM = 300, 30, 28, 12
ENDS = slice(30, 42)                 # six pairs at each genome end
ELSEWHERE = slice(42, 42 + N_ELSEWHERE)
FIXED = slice(70, 70 + 2 * len(FIXED_PAIRS))
PLAIN = slice(90, N_PAIRS - N_RANDOM)          # concordant pairs outside the repeat, lengths 30..150
SETTINGS = ((0, False), (0, True), (3 * N_PAIRS, True))          # (batch_size, multi_hit)
MODES = ("default", "tight", "no_unpaired_ff")
KW = {"default": dict(max_hits=100, rep_seeds=1000, max_effort=15, min_ext=30, max_ext=400, max_reseed=2),
      "tight": dict(max_hits=6, rep_seeds=8, max_effort=2, min_ext=3, max_ext=12, max_reseed=2)}
KW["no_unpaired_ff"] = KW["default"]


def pe_kw(mode, max_frag=500):
    """the paired parameters of a mode, as tests/test_gpu_seed_hits.py sets them: policy (0 = FF, 1 = FR), min / max fragment, overlap, unpaired"""
    ff = mode == "no_unpaired_ff"
    return dict(policy=0 if ff else 1, min_frag=0 if mode == "default" else 150, max_frag=max_frag, overlap=mode != "tight", unpaired=not ff)


def best_approx_paired_ragged_cpu(O, hidx, text, genome_len, mates1, mates2, scheme, aln_type, tables, min_scores, seed_len=22, max_hits=100, rep_seeds=1000,
                                  max_effort=15, max_effort_init=15, min_ext=30, max_ext=400, max_reseed=2, band=31, top_seed=0, batch_size=None, multi_hit=True,
                                  policy=1, min_frag=0, max_frag=500, overlap=True, unpaired=True):
    """mates1 / mates2: lists of uint8 arrays in their ORIGINAL orientation; tables[m] = (S [R], first [max_reseed + 1, R], filtered [R]) and
    min_scores[m] [R] of mate m: seed_tables and the worst scores of its lengths.  Alignment = (score, pos, sink, rc, mate, paired).
    Every step of a pass -- thresholds, windows, outputs, the reduction -- is pe_steps_cpu's; this function is the loop around them."""
    R, L = len(mates1), seed_len
    reads = (mates1, mates2)
    lens = ([len(r) for r in mates1], [len(r) for r in mates2])
    BATCH = batch_size or R
    max_effort_init = max(max_effort_init, max_effort); max_ext = max(max_ext, max_effort)
    init = [pe.init(int(min_scores[0][r]), int(min_scores[1][r])) for r in range(R)]
    best_a, best_o = [i[0] for i in init], [i[1] for i in init]
    empty = np.zeros((0, 2), dtype=np.uint32)

    def oriented(read, rc):
        return (np.where(read[::-1] < 4, 3 - read[::-1], read[::-1]) if rc else read).astype(np.uint8)

    n_extensions = n_opposite = passes = multi_passes = 0
    for anchor in (0, 1):
        a_reads, o_reads = reads[anchor], reads[1 - anchor]
        a_lens, o_lens = lens[anchor], lens[1 - anchor]
        a_min, o_min = min_scores[anchor], min_scores[1 - anchor]
        S, first, filtered = tables[anchor]
        prm = pe.Params(anchor, SCORE_MIN, pe.WORST_SCORE, scheme.match, scheme.txt_gap_open, scheme.txt_gap_ext, band, genome_len, policy, min_frag, max_frag,
                        1 if overlap else 0, 1 if unpaired else 0, max_effort, min_ext, max_ext)
        queue = list(range(R))
        for seeding_pass in range(max_reseed + 1):
            if not queue:
                break
            # the largest seed count of a read of the BATCH in this pass; 0: no read has a seed slot left, here or in a later pass
            if not any((not filtered[r]) and a_lens[r] >= L + int(first[seeding_pass][r]) for r in range(R)):
                break
            deques, trys, nxt = {}, {}, []
            for r in queue:
                M, S_r, first_r = a_lens[r], int(S[r]), int(first[seeding_pass][r])
                trys[r] = max_effort_init
                if filtered[r]:                                        # not seeded, not reseeded (mapping_inl.h:510-514)
                    deques[r] = empty
                    continue
                if M < L + first_r:                                    # no seed slot in this pass: range_count == 0 -> reseed (:549)
                    deques[r] = empty
                    nxt.append(r)
                    continue
                stored = a_reads[r][::-1]
                seed_off = first_r + np.arange((M - L - first_r) // S_r + 1) * S_r
                seeds = np.concatenate([stored[o:o + L] for o in seed_off]).astype(np.uint8)
                offs = (np.arange(len(seed_off) + 1) * L).astype(np.uint32)
                fw = O.match_batch(hidx, seeds, offs, reverse=True)
                comp = np.where(seeds < 4, 3 - seeds, seeds).astype(np.uint8)
                rc = O.match_batch(hidx, comp, offs)
                deques[r], reseed = O.map_exact_read(fw, rc, seed_off, M, L, max_hits, rep_seeds)
                if reseed:
                    nxt.append(r)
            active = [(r, top_seed) for r in queue]
            n_ext = 0
            while active and n_ext < max_ext:
                n_multi = 1
                if multi_hit and len(active) <= BATCH // 2:
                    n_multi = max(1, min(BATCH // len(active), min(4096, max_ext - n_ext)))
                out = []
                for r, top in active:
                    if trys[r] == 0 or len(deques[r]) == 0:
                        continue
                    hits = []
                    for _ in range(n_multi):
                        ok, row, seed, top, deques[r] = O.select_read(deques[r], top)
                        if not ok:
                            break
                        hits.append((row, seed))
                    if hits:
                        out.append((r, top, hits))
                if not out:
                    break
                # score every selected hit against the state BEFORE this pass's reduction (the streams run before score_reduce)
                scored = []
                for r, top, hits in out:
                    M, Mo = a_lens[r], o_lens[r]
                    a_worst, o_worst, o_opt = int(a_min[r]), int(o_min[r]), scheme.match * Mo
                    bb = [best_a[r][0], best_a[r][1], best_o[r][0], best_o[r][1]]          # [a1, a2, o1, o2]
                    rows = []
                    for row, seed in hits:
                        pos = int(O.locate_batch(hidx, np.array([row], dtype=np.uint32))[0])
                        g = (pos - (seed & 0xFFF)) & 0xFFFFFFFF
                        rc = (seed >> 13) & 1
                        _, begin, end, ms = pe.anchor_flatten(prm, bb, rc, g, M, a_worst, o_worst, o_opt)
                        s1, sink1 = SCORE_MIN, 0xFFFFFFFF
                        if end > begin:
                            _, s1, k1 = O.banded_gotoh(band, aln_type, scheme, oriented(a_reads[r], rc), text[begin:end])
                            sink1 = k1[0]
                        hit_score, hit_sink, o_score, valid = pe.anchor_output(int(s1), int(sink1), begin, ms, pe.WORST_SCORE)
                        o_loc = o_sink = 0
                        if valid:
                            n_opposite += 1
                            o_flags, obeg, oend, ms2, why = pe.opposite_flatten(prm, bb, rc, g, hit_score, M, Mo, a_worst, o_worst, o_opt)
                            s2, k2 = SCORE_MIN, (0xFFFFFFFF, 0xFFFFFFFF)
                            if why is None:
                                _, s2, k2 = O.full_gotoh(aln_type, 0, scheme, oriented(o_reads[r], 1 if o_flags == pe.READ_COMPLEMENT else 0), text[obeg:oend], None, ms2)
                            o_score, o_loc, o_sink = pe.opposite_output(int(s2), int(k2[0]), obeg, oend, ms2, pe.WORST_SCORE)
                        rows.append((g, hit_sink, hit_score, o_score, o_loc, o_sink, rc, (seed >> 14) & 1))
                    scored.append(rows)
                # score_reduce_paired
                for (r, top, hits), rows in zip(out, scored):
                    best_a[r], best_o[r], trys[r], erase, _ = pe.reduce_read(prm, [best_a[r][0], best_a[r][1], best_o[r][0], best_o[r][1]], trys[r], rows, a_lens[r], n_ext)
                    if erase:
                        deques[r] = deques[r][:0]
                    n_extensions += len(rows)
                n_ext += n_multi; passes += 1; multi_passes += (n_multi > 1)
                active = [(r, top) for r, top, _ in out]
            queue = nxt
    return dict(best_a=np.array(best_a, dtype=np.int64), best_o=np.array(best_o, dtype=np.int64), n_extensions=n_extensions, n_opposite=n_opposite, passes=passes,
                multi_passes=multi_passes)


def paired_genome(rng, G=300_000):
    """the genome of tests/test_gpu_seed_hits.py's paired test: random, with a 12-copy repeat long enough to hold whole fragments"""
    text = rng.integers(0, 4, G, dtype=np.uint8)
    unit = rng.integers(0, 4, 600, dtype=np.uint8)
    for c in range(12):
        text[40000 + 5000 * c:40600 + 5000 * c] = unit
        for _ in range(3):
            text[40000 + 5000 * c + int(rng.integers(0, 600))] = rng.integers(0, 4)
    return text


def make_pairs(rng, text, starts, frag, len1, len2, ff, exact, elsewhere=(), random1=(), random2=()):
    """FR: mate 1 forward at the fragment's start and mate 2 reverse-complemented at its end -- or, the fragment read from the other strand, mate 1
    reverse-complemented at the end and mate 2 forward at the start; FF: both forward, mate 1 upstream.  3 % substitutions and a few N except in the
    `exact` pairs; mate 2 of `elsewhere` lies at a random place; the mates of random1 / random2 are random symbols.  -> (mates1, mates2): lists"""
    G, R = len(text), len(starts)
    flip = (rng.random(R) < 0.5) & (not ff)
    m1, m2 = [], []
    for r in range(R):
        L1, L2, s, f = int(len1[r]), int(len2[r]), int(starts[r]), int(frag[r])
        p1, p2 = (s + f - L1, s) if flip[r] else (s, s + f - L2)
        if r in elsewhere:
            p2 = int(rng.integers(0, G - L2))
        pair = []
        for p, M, rc in ((p1, L1, bool(flip[r])), (p2, L2, (not flip[r]) and not ff)):
            a = text[p:p + M].copy() if r in exact else mutate_reads(rng, text, np.array([p]), M, sub=0.03)[0]
            if rc:
                a = (3 - a[::-1]).astype(np.uint8)
            if r not in exact:
                a[rng.random(M) < 0.002] = 4
            pair.append(a)
        if r in random1:
            pair[0] = rng.integers(0, 4, L1, dtype=np.uint8)
        if r in random2:
            pair[1] = rng.integers(0, 4, L2, dtype=np.uint8)
        m1.append(np.ascontiguousarray(pair[0])); m2.append(np.ascontiguousarray(pair[1]))
    return m1, m2


_SHARED = {}


def genome_and_index(O):
    if "genome" not in _SHARED:
        text = paired_genome(np.random.default_rng(47))
        _SHARED["genome"] = (text, O.build_index(text))
    return _SHARED["genome"]


def shared_input(O, ff):
    """-> (text, hidx, mates1, mates2): N_PAIRS pairs, mate lengths drawn independently from 30..150, fragments 230..480 or as long as the longer mate:
    pairs 0..30 inside the repeat, ENDS at the two genome ends, ELSEWHERE with the second mate at a random place, FIXED = two pairs of every length pair
    of FIXED_PAIRS (the first an exact copy), the last N_RANDOM with a random mate 2 (the last 8 of them also a random mate 1)"""
    key = ("in", ff)
    if key not in _SHARED:
        text, hidx = genome_and_index(O)
        rng = np.random.default_rng(4711)
        G, R = len(text), N_PAIRS
        len1, len2 = rng.integers(30, 151, R), rng.integers(30, 151, R)
        for k, (a, b) in enumerate(FIXED_PAIRS):
            len1[FIXED.start + 2 * k:FIXED.start + 2 * k + 2] = a
            len2[FIXED.start + 2 * k:FIXED.start + 2 * k + 2] = b
        frag = np.maximum(rng.integers(230, 480, R), np.maximum(len1, len2))
        starts = rng.integers(0, G - 1100, R)
        starts[:N_REPEAT] = 40000 + 5000 * rng.integers(0, 12, N_REPEAT) + rng.integers(0, 100, N_REPEAT)
        starts[30:36] = rng.integers(0, 5, 6); starts[36:42] = G - frag[36:42] - rng.integers(0, 4, 6)
        m1, m2 = make_pairs(rng, text, starts, frag, len1, len2, ff, exact=set(range(FIXED.start, FIXED.stop, 2)),
                            elsewhere=set(range(ELSEWHERE.start, ELSEWHERE.stop)), random1=set(range(R - 8, R)), random2=set(range(R - N_RANDOM, R)))
        _SHARED[key] = (text, hidx, m1, m2)
    return _SHARED[key]


def long_input(O):
    """four pairs whose 1023-symbol mates can pair under max_frag_len = 1500 -> (text, hidx, mates1, mates2); the first two are exact copies"""
    if "long" not in _SHARED:
        text, hidx = genome_and_index(O)
        rng = np.random.default_rng(4712)
        len1, len2 = np.array([1023, 100, 1023, 600]), np.array([100, 1023, 1023, 1023])
        frag = np.array([1200, 1100, 1400, 1300])
        starts = np.array([100_000, 150_000, 200_000, 250_000]) + rng.integers(0, 1000, 4)
        m1, m2 = make_pairs(rng, text, starts, frag, len1, len2, False, exact={0, 1})
        _SHARED["long"] = (text, hidx, m1, m2)
    return _SHARED["long"]


def tables_of(m1, m2):
    """-> (tables, min_scores): per mate (S, first, filtered) and the end-to-end worst scores of its lengths"""
    lens = [np.array([len(r) for r in m]) for m in (m1, m2)]
    return [seed_tables(l) for l in lens], [np.array([min_score_e2e(M) for M in l], dtype=np.int32) for l in lens]


def min_score_local(M):
    """nvBowtie's local threshold int( 10 ln M ) in float32 (MinScoreFunc, scoring.h:117-129), as pipeline.SeedExtendParams.min_score_for"""
    import math
    return int(np.float32(0.0) + np.float32(10.0) * np.float32(math.log(np.float32(M))))


def restatement(O, mode, batch_size, multi_hit, which="shared", max_frag=500, local=False, pairs=None):
    """best_approx_paired_ragged_cpu over the shared (or the long) input in one mode and setting, computed once per process.  local: nvBowtie's local
    scheme (match 2), LOCAL alignment and the thresholds int( 10 ln M ) instead of the end-to-end ones; pairs: a slice of the input"""
    import oracle
    key = ("want", mode, batch_size, multi_hit, which, max_frag, local, None if pairs is None else (pairs.start, pairs.stop))
    if key not in _SHARED:
        text, hidx, m1, m2 = shared_input(O, mode == "no_unpaired_ff") if which == "shared" else long_input(O)
        if pairs is not None:
            m1, m2 = m1[pairs], m2[pairs]
        tables, min_scores = tables_of(m1, m2)
        scheme, aln_type = oracle.Scheme(0, 6, 6, -8, -3, -8, -3), oracle.SEMI_GLOBAL
        if local:
            scheme, aln_type = oracle.Scheme(2, 2, 6, -8, -3, -8, -3), oracle.LOCAL
            min_scores = [np.array([min_score_local(len(r)) for r in m], dtype=np.int32) for m in (m1, m2)]
        _SHARED[key] = best_approx_paired_ragged_cpu(O, hidx, text, len(text), m1, m2, scheme, aln_type, tables, min_scores,
                                                     batch_size=batch_size or None, multi_hit=multi_hit, **pe_kw(mode, max_frag), **KW[mode])
    return _SHARED[key]
