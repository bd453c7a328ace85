"""Test infrastructure: nvBowtie's best-approx single-end loop over reads of DIFFERENT lengths, restated pass by pass over the whole batch with
the several-hits-per-read phase, on the oracle's per-read pieces (O.map_exact_read, O.select_read, O.score_reduce_effort, O.banded_gotoh,
O.locate_batch).  It is oracle/cpu_pipeline.nvbowtie_best_approx_batch_cpu with every quantity the reference's map_kernel computes per lane
(mapping_inl.h:504-529) made per read: the length M_r, the seed interval S_r, the first seed offset of a pass first_r, the worst score.

The contract it restates (include/nvbio_amd.h, "reads of DIFFERENT lengths"):
  * seeds of read r in a pass at stored offsets first_r + j * S_r while first_r + j * S_r + L <= M_r;
  * a read with M_r < max( min_read_len, L ) is filtered: an empty deque in every pass, never queued for reseeding, unaligned at the end
    (the reference would seed a read with min_read_len <= M_r < L once with the whole read: the library's one divergence);
  * a read that passed the filter but has no seed slot in a pass gets an empty deque and is queued for reseeding (range_count == 0);
  * the forward hit's pos_in_read, the DP window end and the distinct distance use M_r; n_multi is a batch-wide number.
Also here: the ragged input the CPU and GPU tests share, and its per-read tables."""
import numpy as np

from oracle.cpu_pipeline import SCORE_MIN
from util import mutate_reads

FIXED_LENGTHS = (11, 21, 22, 23, 30, 49, 50, 99, 100, 101, 149, 150, 151, 250, 1023)
N_RANDOM = 15
KW = {"default": dict(max_hits=100, rep_seeds=1000, max_effort=15, min_ext=30, max_ext=400, max_reseed=2),
      "tight": dict(max_hits=6, rep_seeds=8, max_effort=2, min_ext=3, max_ext=12, max_reseed=2)}


def seed_freq_of(lens, seed_freq=None):
    """seed_freq( read_len ) = int32( 1 + 1.15f * sqrtf( len ) ) (SimpleFunc, params.h:87-100), in float32 as the reference evaluates it"""
    lens = np.asarray(lens)
    if seed_freq:
        return np.full(len(lens), seed_freq, dtype=np.int64)
    return np.maximum((np.float32(1.0) + np.float32(1.15) * np.sqrt(lens.astype(np.float32))).astype(np.int64), 1)


def seed_tables(lens, seed_len=22, seed_freq=None, max_reseed=2, min_read_len=12):
    """-> (S [R], first [max_reseed + 1, R], filtered [R]) of the contract"""
    lens = np.asarray(lens, dtype=np.int64)
    S = seed_freq_of(lens, seed_freq)
    first = np.stack([p * (S // (max_reseed + 1)) for p in range(max_reseed + 1)])
    return S, first, lens < max(min_read_len, seed_len)


def best_approx_ragged_cpu(O, hidx, text, genome_len, reads, scheme, aln_type, S, first, filtered, min_scores, seed_len=22, max_hits=100, rep_seeds=1000,
                           max_effort=15, max_effort_init=15, min_ext=30, max_ext=400, max_reseed=2, band=31, top_seed=0, batch_size=None, multi_hit=True):
    """reads: a list of uint8 arrays in their ORIGINAL orientation (M_r = len(reads[r])); S [R], first [max_reseed + 1, R], filtered [R],
    min_scores [R]: every read's seed interval, first seed offset per seeding pass, filter decision and worst score."""
    R, L = len(reads), seed_len
    lens = [len(r) for r in reads]
    max_effort_init = max(max_effort_init, max_effort); max_ext = max(max_ext, max_effort)
    BATCH = batch_size or R
    best = np.zeros((R, 6), dtype=np.int64)
    best[:, 0] = min_scores; best[:, 3] = min_scores; best[:, 1] = 0xFFFFFFFF; best[:, 4] = 0xFFFFFFFF
    n_extensions = passes = multi_passes = 0
    empty = np.zeros((0, 2), dtype=np.uint32)
    queue = list(range(R))
    for seeding_pass in range(max_reseed + 1):
        if not queue:
            break
        deques, trys, nxt = {}, {}, []
        for r in queue:
            M, S_r, first_r = lens[r], int(S[r]), int(first[seeding_pass][r])
            trys[r] = max_effort_init
            if filtered[r]:                                            # `read_len < params.min_read_len` (mapping_inl.h:510-514): dropped, not reseeded
                deques[r] = empty
                continue
            if M < L + first_r:                                        # no seed slot in this pass: range_count == 0 -> reseed (:549)
                deques[r] = empty
                nxt.append(r)
                continue
            stored = reads[r][::-1]
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
                    if trys[r] != 0:
                        deques[r] = deques[r][:0]
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
            for r, top, hits in out:
                M = lens[r]
                b = list(best[r]); erase_any = False
                fwd = reads[r].astype(np.uint8)
                rcp = np.where(reads[r][::-1] < 4, 3 - reads[r][::-1], reads[r][::-1]).astype(np.uint8)
                for idx, (row, seed) in enumerate(hits):
                    pos = int(O.locate_batch(hidx, np.array([row], dtype=np.uint32))[0])
                    g_pos = (pos - (seed & 0xFFF)) & 0xFFFFFFFF
                    read_rc = (seed >> 13) & 1
                    begin = g_pos - band // 2 if g_pos > band // 2 else 0
                    end = min((begin + band + M) & 0xFFFFFFFF, genome_len)
                    if end > begin:
                        _, score, _ = O.banded_gotoh(band, aln_type, scheme, rcp if read_rc else fwd, text[begin:end])
                    else:
                        score = SCORE_MIN
                    score = max(score, -65536)
                    b, trys[r], erase = O.score_reduce_effort(b, trys[r], score, g_pos, read_rc, (seed >> 14) & 1, M, n_ext + idx, max_effort, min_ext, max_ext)
                    erase_any = erase_any or erase
                best[r] = b
                if erase_any:
                    deques[r] = deques[r][:0]
                n_extensions += len(hits)
            n_ext += n_multi; passes += 1; multi_passes += (n_multi > 1)
            active = [(r, top) for r, top, _ in out]
        queue = nxt
    return dict(best_score=best[:, 0].astype(np.int32), best_loc=np.where(best[:, 1] == 0xFFFFFFFF, -1, best[:, 1]), best_rc=best[:, 2].astype(np.uint8),
                second_score=best[:, 3].astype(np.int32), second_loc=np.where(best[:, 4] == 0xFFFFFFFF, -1, best[:, 4]),
                second_rc=best[:, 5].astype(np.uint8), n_extensions=n_extensions, passes=passes, multi_passes=multi_passes)


def repeat_genome(rng, G=400_000):
    """the genome of tests/test_gpu_seed_hits.py's loop test: random, with a 30-copy repeat (wide ranges, the cap, the effort limit)"""
    text = rng.integers(0, 4, G, dtype=np.uint8)
    unit = rng.integers(0, 4, 250, dtype=np.uint8)
    for c in range(30):
        text[50000 + 4000 * c:50250 + 4000 * c] = unit
        text[50000 + 4000 * c + int(rng.integers(0, 250))] = rng.integers(0, 4)
    return text


_SHARED = {}


def shared_input():
    """-> (text, reads): a 400 k genome with the 30-copy repeat and 600 reads in their original orientation (a list of uint8 arrays): 200 inside the
    repeat, 10 at each genome end, four of every length of FIXED_LENGTHS (two of them exact copies), the rest 100..150 long; 3 % substitutions, a few N, half of them
    reverse-complemented; the last N_RANDOM reads random (unalignable)"""
    if "in" not in _SHARED:
        rng = np.random.default_rng(2031)
        text = repeat_genome(rng)
        G, R = len(text), 600
        lens = rng.integers(100, 151, R)
        lens[230:230 + 4 * len(FIXED_LENGTHS)] = np.repeat(FIXED_LENGTHS, 4)
        starts = rng.integers(0, G - 1100, R)
        starts[:200] = 50000 + 4000 * rng.integers(0, 30, 200) + rng.integers(0, 90, 200)
        starts[200:210] = rng.integers(0, 6, 10); starts[210:220] = G - lens[210:220] - 8 - rng.integers(0, 4, 10)
        reads = []
        for r in range(R):
            M = int(lens[r])
            a = mutate_reads(rng, text, starts[r:r + 1], M, sub=0.03)[0]
            exact = 230 <= r < 230 + 4 * len(FIXED_LENGTHS) and (r - 230) % 4 < 2      # two of every fixed length are exact copies: a one-seed read can hit
            if exact:
                a = text[starts[r]:starts[r] + M].copy()
            if rng.random() < 0.5:
                a = (3 - a[::-1]).astype(np.uint8)
            if not exact:
                a[rng.random(M) < 0.002] = 4
            if r >= R - N_RANDOM:
                a = rng.integers(0, 4, M, dtype=np.uint8)
            reads.append(np.ascontiguousarray(a))
        _SHARED["in"] = (text, reads)
    return _SHARED["in"]


def stored_stream(reads):
    """the batch as nvBowtie stores it: every read reversed, back to back -> (symbols uint8, offsets uint32 [R + 1])"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint32)
    return np.concatenate([r[::-1] for r in reads]).astype(np.uint8), off


def per_read_oracle(O, cpu_pipeline, hidx, text, reads, scheme, aln_type, min_scores, filtered, **kw):
    """cpu_pipeline.nvbowtie_best_approx_cpu called once per read at that read's own length and worst score (one hit per read and pass): the
    ragged reference.  A filtered read is not handed over -- the oracle would seed it with the whole read -- and stays unaligned."""
    R = len(reads)
    out = dict(best_score=np.array(min_scores, dtype=np.int32), best_loc=np.full(R, -1, dtype=np.int64), best_rc=np.zeros(R, dtype=np.uint8),
               second_score=np.array(min_scores, dtype=np.int32), second_loc=np.full(R, -1, dtype=np.int64), second_rc=np.zeros(R, dtype=np.uint8), n_extensions=0)
    for r in range(R):
        if filtered[r]:
            continue
        one = cpu_pipeline.nvbowtie_best_approx_cpu(O, hidx, text, len(text), reads[r][None, :], scheme, aln_type, int(min_scores[r]), **kw)
        for k in ("best_score", "best_loc", "best_rc", "second_score", "second_loc", "second_rc"):
            out[k][r] = one[k][0]
        out["n_extensions"] += one["n_extensions"]
    return out


def references(O, mode):
    """the references of one parameter set over the shared input, computed once per process:
    -> dict(hidx, min_scores, S, first, filtered, per_read, multi = {batch_size: restatement})"""
    import oracle
    from oracle import cpu_pipeline
    key = ("ref", mode)
    if key not in _SHARED:
        text, reads = shared_input()
        hidx = _SHARED.get("hidx")
        if hidx is None:
            hidx = _SHARED["hidx"] = O.build_index(text)
        lens = np.array([len(r) for r in reads])
        S, first, filtered = seed_tables(lens)
        min_scores = np.array([min_score_e2e(M) for M in lens], dtype=np.int32)
        osc = oracle.Scheme(0, 6, 6, -8, -3, -8, -3)
        kw = KW[mode]
        per_read = per_read_oracle(O, cpu_pipeline, hidx, text, reads, osc, oracle.SEMI_GLOBAL, min_scores, filtered, **kw)
        multi = {bs: best_approx_ragged_cpu(O, hidx, text, len(text), reads, osc, oracle.SEMI_GLOBAL, S, first, filtered, min_scores, batch_size=bs or None, **kw)
                 for bs in (0, 3 * len(reads))}
        _SHARED[key] = dict(hidx=hidx, min_scores=min_scores, S=S, first=first, filtered=filtered, per_read=per_read, multi=multi)
    return _SHARED[key]


def min_score_e2e(M):
    """nvBowtie's end-to-end threshold: linear -0.6 - 0.6 L in float32 (scoring_inl.h:99-114, MinScoreFunc scoring.h:117-129)"""
    return int(np.float32(-0.6) + np.float32(-0.6) * np.float32(max(M, 1)))
