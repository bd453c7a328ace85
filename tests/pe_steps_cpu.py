"""A plain-Python restatement of the six data-parallel steps of nvBowtie's PAIRED-END best-approx loop (include/nvbio_amd.h: the block above
nvbio_pe_params and the one above nvbio_pe_ragged) -- init, anchor flatten, anchor output, opposite flatten, opposite output, reduce -- written from
the header and the reference lines it cites, not from the kernels:
  BestAnchorScoreStream / BestOppositeScoreStream     nvBowtie/bowtie2/cuda/score_inl.h:143-274, :283-456
  frame_opposite_mate, compute_target_score           nvBowtie/bowtie2/cuda/alignment_utils.h:52-102
  score_reduce_paired_kernel, ReduceBestApproxContext nvBowtie/bowtie2/cuda/reduce_inl.h:157-290, reduce.h:55-99
  io::Alignment, BestPairedAlignments, distinct_alignments      nvbio/io/alignments.h, alignments_inl.h
  aln::max_text_gaps                                  nvbio/alignment/utils_inl.h:145-167
One function per step, called per hit or per read, over unbounded Python integers; the places where the REFERENCE's variable is uint32 or int32 are
wrapped explicitly and marked `uint32` / `int32`.  The tests compare every output array of the library with these functions; the loop restatement
(best_approx_paired_ragged_cpu.py) is built from them, which ties them to the oracle on every input a real genome produces.

An alignment is the tuple (score, position, sink offset, rc, mate, paired); a read pair's state is b = [a1, a2, o1, o2]
(best_a[r] = (a1, a2), best_o[r] = (o1, o2)).  The library keeps the sink offset in a whole word where the reference has a 10-bit field.

The library's departures from the reference, as the header states them:
  * the term `context->min_score > a_optimal_score` of BestAnchorScoreStream::init_context reads an uninitialised variable: taken as false;
  * a skipped anchor hit gets the window (0, 0) and min_score = INT32_MAX; so does (the window alone) an anchor hit whose window begins at or past
    genome_len or ends before it begins;
  * an opposite job that cannot run gets the window (0, 0), so nvbio_pe_opposite_output reports worst_score and loc = sink = 0 for it, whatever
    score the job's slot holds; `end < begin` after the uint32 arithmetic means "not run" as well."""
from collections import namedtuple

U32 = 0xFFFFFFFF
NONE = U32                                # position of an alignment that is none
INT32_MAX = 0x7FFFFFFF
SCORE_MIN = -(1 << 30)                    # NVBIO_SCORE_MIN: what the library's loop passes as score_limit
WORST_SCORE = -65536                      # scheme_type::worst_score
READ_REVERSE, READ_COMPLEMENT = 1, 2      # reads are stored reversed: forward = REVERSE, reverse-complemented = COMPLEMENT
FF, FR, RF, RR = 0, 1, 2, 3               # NVBIO_PE_POLICY_*

BRANCHES = ("held", "best", "second", "unpaired-best", "unpaired-second", "unpaired-fail", "unpaired-keep", "fail", "keep")
REASONS = ("threshold", "outside", "visited", "empty", "wrapped")

# what nvbio_pe_params holds beside the lengths and the length-derived scores
Params = namedtuple("Params", "anchor score_limit worst_score match txt_gap_open txt_gap_ext band genome_len policy min_frag max_frag overlap unpaired "
                              "max_effort min_ext max_ext")


def u32(v):
    return v & U32


def i32(v):
    return ((v + (1 << 31)) & U32) - (1 << 31)


def tdiv(a, b):
    """C division: truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ---- io::Alignment / BestPairedAlignments ------------------------------------------------------------------------------------------
def aln(score, pos, sink, rc, mate, paired):
    return (score, pos, sink, 1 if rc else 0, mate, 1 if paired else 0)


def flags_word(a):
    """the fourth word of the library's alignment: rc | mate << 1 | paired << 2"""
    return a[3] | (a[4] << 1) | (a[5] << 2)


def is_paired(a):
    return a[5] == 1 and a[1] != NONE                                # m_paired && is_aligned()


def best_score(b):
    return b[0][0] + (b[2][0] if is_paired(b[0]) else 0)


def second_score(b):
    return b[1][0] + (b[3][0] if is_paired(b[1]) else 0)


def init(min_score_mate1, min_score_mate2):
    """init_alignments( reads1, threshold, best_data, 0 ) / ( reads2, ..., best_data_o, 1 ): io::Alignment( -1, max_ed, worst, mate ) -- the fourth
    constructor argument is `rc`, so `mate` lands in the strand slot of best_o -> (best_a[r], best_o[r])"""
    a = aln(min_score_mate1, NONE, 255, 0, 0, False)
    o = aln(min_score_mate2, NONE, 255, 1, 0, False)
    return (a, a), (o, o)


# ---- alignment_utils.h --------------------------------------------------------------------------------------------------------------
def target_score(b, a_worst, o_worst):
    """compute_target_score (alignment_utils.h:93-102)"""
    if not is_paired(b[1]):                                          # has_second_paired()
        return a_worst + o_worst
    delta = i32(best_score(b) - second_score(b))                     # int32
    return i32(second_score(b) + tdiv(i32(delta * 3), 4))            # int32, C truncating division


def frame(policy, anchor, anchor_fw):
    """frame_opposite_mate (alignment_utils.h:52-88) -> (left, fw)"""
    anchor_1 = anchor == 0
    if policy == FF:
        return anchor_1 != anchor_fw, anchor_fw
    if policy == RR:
        return anchor_1 == anchor_fw, anchor_fw
    if policy == FR:
        return not anchor_fw, not anchor_fw
    return anchor_fw, not anchor_fw                                  # RF


def visited(b, mate, rc, g):
    """`skip locations that we have already visited` (score_inl.h:240-244, :431-435) without its last term"""
    return any(mate == x[4] and rc == x[3] and g == x[1] for x in b)


def max_text_gaps(match, txt_gap_open, txt_gap_ext, min_score, pattern_len):
    """aln::max_text_gaps (utils_inl.h:145-167) as its caller stores it: the uint32 n - 1 in an int32, so -1 when the loop does not turn"""
    score = pattern_len * match
    if score < min_score:
        return 0
    score += txt_gap_open
    n = 0
    while score >= min_score and n < pattern_len:
        score += txt_gap_ext
        n += 1
    return i32(u32(n - 1))                                           # uint32 n - 1 -> int32 max_ref_gaps


# ---- BestAnchorScoreStream ----------------------------------------------------------------------------------------------------------
def anchor_window(g, band, a_len, genome_len):
    """score_inl.h:238-239 -> (begin, end) as the reference computes them"""
    begin = u32(g - band // 2) if g > band // 2 else 0               # uint32
    end = min(u32(u32(begin + band) + a_len), genome_len)            # uint32
    return begin, end


def anchor_flatten(p, b, rc, g, a_len, a_worst, o_worst, o_opt):
    """init_context of one selected hit (score_inl.h:200-252) -> (flags, win_begin, win_end, min_score)"""
    target_pair = target_score(b, a_worst, o_worst)
    target_mate = max(i32(target_pair - o_opt), a_worst)             # int32
    skip = visited(b, p.anchor, rc, g)                               # (the uninitialised term: false)
    begin, end = anchor_window(g, p.band, a_len, p.genome_len)
    if skip or begin >= p.genome_len or end < begin:                 # the library: the empty window
        begin = end = 0
    min_score = INT32_MAX if skip else max(target_mate + 1, p.score_limit)
    return (READ_COMPLEMENT if rc else READ_REVERSE), begin, end, min_score


def anchor_output(score, sink_x, win_begin, min_score, worst_score):
    """output (score_inl.h:256-269) and the fill of the opposite scores behind it -> (hit.score, hit.sink, hit.opposite_score, valid);
    valid = the anchor passed with a score other than worst_score: the hits whose opposite mate is aligned next"""
    passed = score >= min_score
    hit_score = score if passed else worst_score
    hit_sink = u32(win_begin + sink_x)                               # uint32
    return hit_score, hit_sink, worst_score, 1 if passed and hit_score != worst_score else 0


# ---- BestOppositeScoreStream --------------------------------------------------------------------------------------------------------
def opposite_frame_window(g, left, a_len, o_gapped, min_frag, max_frag, overlap, genome_len):
    """score_inl.h:401-416, every sum and difference in uint32 as there -> (begin, end), not yet tested against anything"""
    if left:
        reach = u32(u32(g + a_len) + o_gapped)                       # uint32
        max_end = u32(reach - min_frag) if reach > min_frag else 0   # uint32
        begin = u32(u32(g + a_len) - max_frag) if u32(g + a_len) > max_frag else 0       # uint32
        end = u32(g + a_len) if overlap else g                       # uint32
        end = min(end, max_end)
    else:
        min_begin = u32(u32(g + min_frag) - o_gapped) if u32(g + min_frag) > o_gapped else 0     # uint32
        end = u32(g + max_frag)                                      # uint32
        begin = g if overlap else u32(g + a_len)                     # uint32
        begin = max(begin, min_begin)
    return begin, min(end, genome_len)


def opposite_flatten(p, b, rc, g, anchor_score, a_len, o_len, a_worst, o_worst, o_opt):
    """init_context of one hit whose anchor passed (score_inl.h:330-440) -> (flags, win_begin, win_end, min_score, reason); reason = None for
    a job that runs, else the first of REASONS that keeps it from running (its window is then (0, 0))"""
    target_pair = target_score(b, a_worst, o_worst)
    target_mate = max(i32(target_pair - anchor_score), o_worst)      # int32
    min_score = max(target_mate + 1, p.score_limit)
    left, fw = frame(p.policy, p.anchor, rc == 0)
    o_rc = 0 if fw else 1
    max_ref_gaps = max_text_gaps(p.match, p.txt_gap_open, p.txt_gap_ext, min_score, o_len)       # int32
    o_gapped = u32(o_len + max_ref_gaps)                             # uint32
    begin, end = opposite_frame_window(g, left, a_len, o_gapped, p.min_frag, p.max_frag, p.overlap, p.genome_len)
    reason = None
    if min_score > o_opt:
        reason = "threshold"
    elif begin >= p.genome_len:
        reason = "outside"
    elif visited(b, 0 if p.anchor else 1, o_rc, g):
        reason = "visited"
    elif begin == end:
        reason = "empty"
    elif end < begin:                                                # the library: a window that wrapped
        reason = "wrapped"
    if reason:
        begin = end = 0
    return (READ_COMPLEMENT if o_rc else READ_REVERSE), begin, end, min_score, reason


def opposite_output(score, sink_x, win_begin, win_end, min_score, worst_score):
    """output (score_inl.h:444-456) -> (hit.opposite_score, hit.opposite_loc, hit.opposite_sink); a job that did not run (no window) reports
    worst_score whatever its slot holds"""
    ran = win_end > win_begin
    genome_sink = sink_x if sink_x != U32 else 0
    return (score if ran and score >= min_score else worst_score), win_begin, u32(win_begin + genome_sink)        # uint32


# ---- distinct_alignments ------------------------------------------------------------------------------------------------------------
def distinct(pos1, rc1, pos2, rc2, dist):
    """alignments_inl.h:26-38, positions uint32"""
    if rc1 != rc2:
        return True
    return not (pos1 >= u32(pos2 - min(pos2, dist)) and pos1 <= u32(pos2 + dist))       # uint32


def pair_mate(a, o, m):
    """PairedAlignments::mate (alignments.h:197-200)"""
    return a if m == a[4] else o


def pairs_distinct(a1, o1, a2, o2, dist=None):
    """distinct_alignments of two pairs (alignments_inl.h:44-110): on the END positions of mate 0 and of mate 1, exactly (dist None) or within dist"""
    p10, p11, p20, p21 = pair_mate(a1, o1, 0), pair_mate(a1, o1, 1), pair_mate(a2, o2, 0), pair_mate(a2, o2, 1)
    ap1, op1, ap2, op2 = u32(p10[1] + p10[2]), u32(p11[1] + p11[2]), u32(p20[1] + p20[2]), u32(p21[1] + p21[2])      # uint32
    if dist is None:
        return p10[3] != p20[3] or p11[3] != p21[3] or ap1 != ap2 or op1 != op2
    if p10[3] != p20[3] or p11[3] != p21[3]:
        return True
    near = lambda x, y: x >= u32(y - min(y, dist)) and x <= u32(y + dist)                # uint32
    return not (near(ap1, ap2) and near(op1, op2))


# ---- score_reduce_paired_kernel -----------------------------------------------------------------------------------------------------
def reduce_read(p, b, trys, hits, a_len, ext):
    """one read's hits in selection order (reduce_inl.h:175-290).  hits: rows (loc, sink, score, opposite_score, opposite_loc, opposite_sink, rc,
    top_flag).  -> (best_a[r], best_o[r], trys, erased, branches): the state as MEMORY holds it afterwards, the try counter, whether the read's
    deque was erased (sizes[r] = 0) and the branch every hit took.
    The reference keeps a local copy `best_pairs` that a paired update changes together with memory, while an unpaired update writes memory alone
    (:262-273): later hits of the same list do not see the unpaired updates, and a later paired update writes the local copy over them."""
    local = list(b)
    memory = list(b)
    dist = a_len // 2
    anchor = p.anchor
    erased = False
    branches = []

    def failure(idx, top_flag):                                      # reduce.h:82-92
        nonlocal trys
        if trys > 0:
            if u32(ext + idx) >= p.min_ext and top_flag == 0:        # uint32
                trys -= 1
                if trys == 0:
                    return True
            if u32(ext + idx) >= p.max_ext:                          # uint32
                return True
        return False

    for idx, (gx, gy, s1, s2, ox, oy, rc, top_flag) in enumerate(hits):
        score = i32(s1 + s2)                                         # int32
        _, o_fw = frame(p.policy, anchor, rc == 0)
        o_rc = 0 if o_fw else 1
        pa = aln(s1, gx, u32(gy - gx), rc, anchor, True)             # uint32 g_pos.y - g_pos.x
        po = aln(s2, ox, u32(oy - ox), o_rc, 1 - anchor, True)       # uint32
        a1, a2, o1, o2 = local
        if not pairs_distinct(a1, o1, pa, po) or not pairs_distinct(a2, o2, pa, po):
            branches.append("held")
        elif score > best_score(local):
            trys = p.max_effort
            local = [pa, a1, po, o1]
            memory = list(local)
            branches.append("best")
        elif score > second_score(local) and pairs_distinct(a1, o1, pa, po, dist):
            trys = p.max_effort
            local = [a1, pa, o1, po]
            memory = list(local)
            branches.append("second")
        elif p.unpaired and not is_paired(a1):
            m1 = a1 if anchor == a1[4] else o1                       # best_pairs.mate( anchor ) (alignments.h:314-318)
            m2 = a2 if anchor == a2[4] else o2
            wrote = True
            if s1 > m1[0]:
                m1, m2 = aln(s1, gx, u32(gy - gx), rc, anchor, False), m1
                branches.append("unpaired-best")
            elif s1 > m2[0] and distinct(m1[1], m1[3], gx, rc, dist):
                m2 = aln(s1, gx, u32(gy - gx), rc, anchor, False)
                branches.append("unpaired-second")
            else:
                wrote = False
                if failure(idx, top_flag):
                    erased = True
                    branches.append("unpaired-fail")
                else:
                    branches.append("unpaired-keep")
            if wrote:
                if anchor:
                    memory[2], memory[3] = m1, m2
                else:
                    memory[0], memory[1] = m1, m2
        elif failure(idx, top_flag):
            erased = True
            branches.append("fail")
        else:
            branches.append("keep")
    return (memory[0], memory[1]), (memory[2], memory[3]), trys, erased, branches
