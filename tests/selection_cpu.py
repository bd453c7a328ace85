"""A plain-Python restatement of the selection stage -- the index arithmetic between FMIndexFilter::locate and the SAM writer
(include/nvbio_amd.h: "seed hits -> candidate windows", "Best candidate per read ..." to nvbio_opposite_mate_windows, the scoring
stream, the two sw-benchmark conversions) -- written from the header and the reference lines it cites, not from the kernels.  The
tests compare every output array of the library with it.

Everything is computed in unbounded Python integers; the few places where the REFERENCE itself computes in uint32 (and the header
says so) are marked `uint32`.  The `*_np` twins restate the same rule over numpy arrays for the one list too long for a Python loop.

A candidate is (key, score, win_begin, sink_x):
  key = read << 34 | strand << 33 | (diagonal + 1024)        the diagonal key of hits_to_diagonals
  sel = max(score + 2^20, 0) << 34 | strand << 33 | (win_begin + sink_x)        its selection key
"""
import numpy as np

SCORE_MIN = -(1 << 30)
U32 = 0xFFFFFFFF
BIAS = 1024                               # the diagonal field holds diagonal + 1024
FIELD = (1 << 33) - 1                     # the 33-bit position field of both keys
STRAND = 1 << 33
SCORE_BIAS = 1 << 20
RC_FLAGS = 3                              # NVBIO_READ_REVERSE | NVBIO_READ_COMPLEMENT
MAX_SEED_OFFSET = 1024                    # read_len - seed_len at most: beyond it a diagonal can leave the field (see diagonal_field)


# ---- keys -------------------------------------------------------------------------------------------------------------------------
def seed_offset(seed_id, seeds_per_read, seed_interval, seed_len, read_len, strand):
    """offset of seed `seed_id` in its read as the strand reads it (fmmap.cu:92-117 over uniformly enumerated seeds)"""
    p = (seed_id % seeds_per_read) * seed_interval
    return read_len - p - seed_len if strand else p


def diagonal_field(text_pos, p):
    """diagonal + 1024 of a hit at text_pos of a seed at read offset p, as an unbounded integer: it fits the key's 33-bit field iff
    0 <= value < 2^33, which p <= 1024 guarantees for every text_pos below 2^32"""
    return text_pos - p + BIAS


def hit_to_diagonal(text_pos, seed_id, seeds_per_read, seed_interval, seed_len, read_len, strand):
    """the diagonal key of one hit; a diagonal outside the field has no key (ValueError)"""
    rid = seed_id // seeds_per_read
    d = diagonal_field(text_pos, seed_offset(seed_id, seeds_per_read, seed_interval, seed_len, read_len, strand))
    if not 0 <= d <= FIELD:
        raise ValueError("diagonal %d leaves the key's field" % (d - BIAS))
    return (rid << 34) | ((strand & 1) << 33) | d


def hit_to_diagonal_wrapped(text_pos, seed_id, seeds_per_read, seed_interval, seed_len, read_len, strand):
    """what forming the same key in 64-bit unsigned arithmetic WITHOUT the limit gives: a negative field wraps and is OR-ed over the
    strand bit and the read id (the defect the limit MAX_SEED_OFFSET closes; never handed to a kernel)"""
    rid = seed_id // seeds_per_read
    d = diagonal_field(text_pos, seed_offset(seed_id, seeds_per_read, seed_interval, seed_len, read_len, strand)) & ((1 << 64) - 1)
    return (rid << 34) | ((strand & 1) << 33) | d


def key_read(key):
    return key >> 34


def key_strand(key):
    return (key >> 33) & 1


# ---- windows ----------------------------------------------------------------------------------------------------------------------
def window(key, band, read_len, genome_len):
    """genome_infixes with nvBowtie's window rule (fmmap.cu:169-196, score_inl.h:100-106) -> (read, flags, begin, end)"""
    g = max((key & FIELD) - BIAS, 0)                                    # g_pos = max(diagonal, 0)
    begin = g - band // 2 if g > band // 2 else 0
    end = min(begin + band + read_len, genome_len)
    return key_read(key), RC_FLAGS if key_strand(key) else 0, begin, end


def windows(keys, band, read_len, genome_len, read_offsets=None):
    """uniform (read_len) or ragged (read_offsets: every read its own length)"""
    out = []
    for k in keys:
        k = int(k)
        m = int(read_offsets[key_read(k) + 1]) - int(read_offsets[key_read(k)]) if read_offsets is not None else read_len
        out.append(window(k, band, m, genome_len))
    return out


# ---- best, second best, unpack ----------------------------------------------------------------------------------------------------
def selection_key(key, score, win_begin, sink_x):
    return (max(score + SCORE_BIAS, 0) << 34) | (key & STRAND) | (win_begin + sink_x)


def selection_keys(cands):
    return [selection_key(*c) for c in cands]


def best_per_read(cands, n_reads):
    """the largest selection key of every read; 0 without a candidate"""
    best = [0] * n_reads
    for c in cands:
        r = key_read(c[0])
        best[r] = max(best[r], selection_key(*c))
    return best


def best_windows(cands, best, want_locus=True):
    """largest window begin (and locus = max(diagonal, 0)) among the candidates that tie with their read's best on the whole key; -1 = none"""
    wb = [-1] * len(best)
    locus = [-1] * len(best)
    for c in cands:
        r = key_read(c[0])
        if selection_key(*c) == best[r]:
            wb[r] = max(wb[r], c[2])
            locus[r] = max(locus[r], max((c[0] & FIELD) - BIAS, 0))
    return (wb, locus) if want_locus else wb


def unpack(sel):
    """(score, end position, strand) of a best key.  No candidate (key 0): (SCORE_MIN, -1, 0).  A key whose score field is 0 -- every
    score <= -2^20, the scorer's rejected jobs (SCORE_MIN, sink 0xFFFFFFFF) among them -- reports SCORE_MIN, with the position field
    and the strand of the key as they are (for a rejected job: win_begin + 0xFFFFFFFF, no alignment's end)"""
    if sel == 0:
        return SCORE_MIN, -1, 0
    s = sel >> 34
    return (s - SCORE_BIAS if s > 0 else SCORE_MIN), sel & FIELD, (sel >> 33) & 1


def distinct(pos1, rc1, pos2, rc2, dist):
    """io::distinct_alignments (nvbio/io/alignments_inl.h:26-38), positions unbounded"""
    if rc1 != rc2:
        return True
    return not (pos2 - min(pos2, dist) <= pos1 <= pos2 + dist)


def second_per_read(cands, best, dist, worst_score, read_offsets=None, min_scores=None):
    """the largest selection key among a read's candidates that score above the threshold, are not (a copy of) the best and are distinct
    from it; 0 = none.  Ragged: dist = read length // 2 and worst_score = min_scores[read] - 1 of the candidate's own read"""
    second = [0] * len(best)
    for c in cands:
        r = key_read(c[0])
        d = (int(read_offsets[r + 1]) - int(read_offsets[r])) // 2 if read_offsets is not None else dist
        w = int(min_scores[r]) - 1 if min_scores is not None else worst_score
        sel, b = selection_key(*c), best[r]
        if c[1] > w and sel != b and distinct(b & FIELD, (b >> 33) & 1, sel & FIELD, (sel >> 33) & 1, d):
            second[r] = max(second[r], sel)
    return second


def key_score(sel):
    """the score a mapping quality is computed from: the key's score field, unclamped; SCORE_MIN for key 0"""
    return (sel >> 34) - SCORE_BIAS if sel else SCORE_MIN


def mapq(orc, best, second, version, monotone, perfect_score, min_score):
    """(mapq, second score) of one read from its two keys, by the oracle's BowtieMapq2 / BowtieMapq3; a read without a candidate gets 0"""
    ss = key_score(second)
    if best == 0:
        return 0, ss
    return orc.mapq(version, monotone, perfect_score, min_score, key_score(best), second != 0, ss), ss


def mapq_per_read(orc, best, second, version, monotone=None, perfect_score=None, min_score=None, read_offsets=None, min_scores=None, match=0):
    """uniform (monotone, perfect_score, min_score) or ragged: perfect = match x read length, min_scores[read], monotone = (match == 0)"""
    out = []
    for r, (b, s) in enumerate(zip(best, second)):
        if read_offsets is not None:
            out.append(mapq(orc, b, s, version, match == 0, match * (int(read_offsets[r + 1]) - int(read_offsets[r])), int(min_scores[r])))
        else:
            out.append(mapq(orc, b, s, version, monotone, perfect_score, min_score))
    return out


def finish_reads(orc, cands, n_reads, dist, worst_score, version, monotone, perfect_score, min_score, read_offsets=None, min_scores=None, match=0):
    """best + unpack + second best + mapq -> dict of per-read lists, named as the wrapper's outputs"""
    best = best_per_read(cands, n_reads)
    second = second_per_read(cands, best, dist, worst_score, read_offsets, min_scores)
    un = [unpack(b) for b in best]
    mq = mapq_per_read(orc, best, second, version, monotone, perfect_score, min_score, read_offsets, min_scores, match)
    return dict(best=best, second=second, best_score=[u[0] for u in un], best_pos=[u[1] for u in un], best_rc=[u[2] for u in un],
                mapq=[m[0] for m in mq], second_score=[m[1] for m in mq])


# ---- traceback batch --------------------------------------------------------------------------------------------------------------
EMPTY_JOB = (0, 0, 0, SCORE_MIN, (U32, U32))


def traceback_job(best, best_wb, read_len, band, genome_len, min_score):
    """(flags, begin, end, score, sink) of one read's best alignment; the empty job without a candidate or below min_score"""
    score, pos, rc = unpack(best)
    if best == 0 or best_wb < 0 or score < min_score:
        return EMPTY_JOB
    return (RC_FLAGS if rc else 0, best_wb, min(best_wb + band + read_len, genome_len), score, (pos - best_wb, read_len))


def traceback_batch(best, best_wb, read_len, band, genome_len, min_score, read_offsets=None, min_scores=None):
    out = []
    for r in range(len(best)):
        m = int(read_offsets[r + 1]) - int(read_offsets[r]) if read_offsets is not None else read_len
        t = int(min_scores[r]) if min_scores is not None else min_score
        out.append(traceback_job(best[r], best_wb[r], m, band, genome_len, t))
    return out


# ---- opposite-mate window ---------------------------------------------------------------------------------------------------------
def opposite_window(g, anchor_rc, a_len, o_gapped_len, anchor, policy, min_frag, max_frag, overlap, genome_len):
    """BestOppositeScoreStream::init_context with frame_opposite_mate (score_inl.h:389-425, alignment_utils.h:52-88)
    -> (begin, end, flags, valid); an empty window, or one that starts at or past the genome's end, is [0, 0) with valid = 0"""
    anchor_fw, mate1 = not anchor_rc, anchor == 0
    left, fw = {0: (mate1 != anchor_fw, anchor_fw),               # FF
                1: (not anchor_fw, not anchor_fw),                # FR
                2: (anchor_fw, not anchor_fw),                    # RF
                3: (mate1 == anchor_fw, anchor_fw)}[policy]       # RR
    if left:
        max_end = max(g + a_len + o_gapped_len - min_frag, 0)
        begin = max(g + a_len - max_frag, 0)
        end = min(g + a_len if overlap else g, max_end)
    else:
        min_begin = max(g + min_frag - o_gapped_len, 0)
        end = g + max_frag
        begin = max(g if overlap else g + a_len, min_begin)
    end = min(end, genome_len)
    ok = begin < genome_len and begin < end
    return (begin if ok else 0, end if ok else 0, 0 if fw else RC_FLAGS, 1 if ok else 0)


# ---- the scoring stream -----------------------------------------------------------------------------------------------------------
def stream_flatten(idx_queue, hit_read_id, hit_seed, hit_loc, read_index, band, genome_len, reads_reversed):
    """BestScoreStream::init_context per work item (score_inl.h:85-115) -> [(read, flags, begin, end)].  The window's end is
    computed in uint32, as the reference's; a window that begins at or past the genome's end (a locus that wrapped below zero) or
    whose end wrapped below its begin is the empty window [0, 0)"""
    n = len(idx_queue) if idx_queue is not None else len(hit_read_id)
    out = []
    for i in range(n):
        idx = int(idx_queue[i]) if idx_queue is not None else i
        rid, rc, g = int(hit_read_id[idx]), (int(hit_seed[idx]) >> 13) & 1, int(hit_loc[idx])
        m = int(read_index[rid + 1]) - int(read_index[rid])
        begin = g - band // 2 if g > band // 2 else 0
        end = min((begin + band + m) & U32, genome_len)                  # uint32
        if begin >= genome_len or end < begin:
            begin = end = 0
        flags = (2 if rc else 1) if reads_reversed else (RC_FLAGS if rc else 0)
        out.append((rid, flags, begin, end))
    return out


def stream_output(idx_queue, n_hits, scores, sink_x, win_begin, worst):
    """BestScoreStream::output (score_inl.h:119-133) -> {hit: (score, sink)} of the hits the queue names"""
    out = {}
    for i in range(len(scores)):
        idx = int(idx_queue[i]) if idx_queue is not None else i
        out[idx] = (max(int(scores[i]), worst), (int(win_begin[i]) + int(sink_x[i])) & U32)      # uint32
    return out


# ---- the sw-benchmark conversions -------------------------------------------------------------------------------------------------
def le_to_be_word(w):
    """2-bit symbols of one word from little-endian (symbol i at bits [2i, 2i + 2)) to big-endian (bits [30 - 2i, 32 - 2i))"""
    out = 0
    for i in range(16):
        out |= ((w >> (2 * i)) & 3) << (30 - 2 * i)
    return out


def to_int16(v):
    """`int16 = int32`: the low 16 bits, as a signed number"""
    return ((v + (1 << 15)) & 0xFFFF) - (1 << 15)


# ---- numpy twins (the 2^21-candidate list) ----------------------------------------------------------------------------------------
def selection_keys_np(keys, scores, win_begin, sink_x):
    """selection_key over arrays: uint64 holds every field exactly (score field < 2^30, position < 2^33)"""
    s = np.maximum(scores.astype(np.int64) + SCORE_BIAS, 0).astype(np.uint64)
    pos = win_begin.astype(np.uint64) + sink_x.astype(np.uint64)
    return (s << np.uint64(34)) | (keys.astype(np.uint64) & np.uint64(STRAND)) | pos


def best_per_read_np(keys, sel, n_reads):
    best = np.zeros(n_reads, dtype=np.uint64)
    np.maximum.at(best, (keys.astype(np.uint64) >> np.uint64(34)).astype(np.int64), sel)
    return best


def unpack_np(best):
    s = (best >> np.uint64(34)).astype(np.int64)
    score = np.where(s > 0, s - SCORE_BIAS, SCORE_MIN).astype(np.int32)
    pos = np.where(best != 0, (best & np.uint64(FIELD)).astype(np.int64), -1)
    rc = np.where(best != 0, (best >> np.uint64(33)) & np.uint64(1), 0).astype(np.uint8)
    return score, pos, rc
