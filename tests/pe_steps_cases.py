"""The fixed case lists of the paired-end step tests (test_pe_steps_oracle.py proves their coverage on the CPU, test_gpu_pe_steps.py runs the kernels
over them): hits, best states and parameters on every edge of the six steps restated in pe_steps_cpu.py, and the expectations over them.
Every list is built once per process (cached by its configuration), seeded where random, and never modified; every list comes in a UNIFORM form
(one length and one min score per mate) and a RAGGED form (lengths of LENGTHS mixed so that most pairs have a_len != o_len, per-mate min-score tables
that differ for every pair).  Two schemes throughout: nvBowtie's end-to-end scheme (match 0, min score int(-0.6 - 0.6 L)) and its local scheme (match 2,
min score int(10 ln L)); the local lists are run with score_limit = 0 so that the `max( target + 1, score_limit )` term is live, the end-to-end ones
with the NVBIO_SCORE_MIN the library's own loop passes.  None of the kernels reads the text or the reads: a case is index arithmetic only.

A list is a dict: `p` (pe_steps_cpu.Params), per read a_len / o_len (by ROLE), min1 / min2 (by MATE), best (the state [a1, a2, o1, o2]) and per hit
rid / seed (rc << 13 | top_flag << 14) / loc / score, plus what the step needs (queue; active, first, count, trys, ...)."""
import functools
import itertools
import math
from collections import namedtuple

import numpy as np

import pe_steps_cpu as pe

U32 = pe.U32
LENGTHS = (1, 11, 22, 23, 100, 150, 1023)
GENOMES = (1000, 1 << 31, U32)
BAND = 31
MIN_FRAGS, MAX_FRAGS = (0, 150, 5000), (500, 1500, 0)
UNIFORM_PAIRS = ((100, 150), (23, 11), (11, 100), (150, 22))          # (mate 1, mate 2)
COUNTS = (1, 63, 64, 65, 255, 256, 257)
BIG_N = 256 * 8192 + 257                                              # the grid cap of grid_for plus one partial block
POISON = 0x5A5A5A5A

Scheme = namedtuple("Scheme", "name match txt_gap_open txt_gap_ext score_limit")
SCHEMES = {"e2e": Scheme("e2e", 0, -8, -3, pe.SCORE_MIN), "local": Scheme("local", 2, -8, -3, 0)}


def min_score(scheme, length):
    """MinScoreFunc (scoring.h:117-129) in float32: linear -0.6 - 0.6 L end to end, 10 ln L local"""
    if scheme.name == "e2e":
        return int(np.float32(-0.6) + np.float32(-0.6) * np.float32(length))
    return int(np.float32(10.0) * np.float32(math.log(np.float32(length))))


def seed_word(rc, top_flag=0):
    return (rc << 13) | (top_flag << 14)


# ---- the pairs of a list: lengths and min-score tables ------------------------------------------------------------------------------
_PAIRS = [(a, b) for a in LENGTHS for b in LENGTHS]
_PAIRS = [_PAIRS[(i * 11) % len(_PAIRS)] for i in range(len(_PAIRS))]            # mixed: consecutive pairs share no length


def pair_lengths(form, k, uniform_pair):
    """(len of mate 1, len of mate 2) of pair k"""
    return uniform_pair if form == "uniform" else _PAIRS[k % len(_PAIRS)]


def pair_tables(scheme, form, k, len1, len2, permissive):
    """(min score of mate 1, of mate 2): min_score( len ) -- lowered beyond every gap a mate of that length could take where `permissive` (a table
    is an input like any other) -- and never the same number for the two mates of a ragged pair"""
    low = lambda m: 8 + 3 * m + 10
    m1 = min_score(scheme, len1) - (low(len1) if permissive else 0)
    m2 = min_score(scheme, len2) - (low(len2) if permissive else 0)
    if m1 == m2:
        m2 -= 1 + (k % 2 if form == "ragged" else 0)
    return m1, m2


# ---- best states ------------------------------------------------------------------------------------------------------------------
DELTAS = (0, 1, 2, 3, 5, 400, -1, -5)
STATE_KINDS = (["init", "unpaired", "unpaired-other", "pair", "other-anchor", "flipped-o"] + ["two%+d" % d for d in DELTAS] +
               ["vis-a%d" % s for s in range(4)] + ["vis-o%d" % s for s in range(4)] +
               ["near-a-%s" % f for f in ("mate", "rc", "pos")] + ["near-o-%s" % f for f in ("mate", "rc", "pos")])


def make_pair(p, row):
    """the pair score_reduce_paired forms from a hit row (loc, sink, score, oscore, oloc, osink, rc, top)"""
    gx, gy, s1, s2, ox, oy, rc, _ = row
    _, o_fw = pe.frame(p.policy, p.anchor, rc == 0)
    return pe.aln(s1, gx, pe.u32(gy - gx), rc, p.anchor, True), pe.aln(s2, ox, pe.u32(oy - ox), 0 if o_fw else 1, 1 - p.anchor, True)


def make_state(kind, p, g, rc, a_len, o_len, min1, min2, base=7777):
    """[a1, a2, o1, o2] of a kind; positions lie `base` and 2 * base past g (so never at g) unless the kind puts one there"""
    a_worst, o_worst = (min2, min1) if p.anchor else (min1, min2)
    sa, so = (a_worst + p.match * a_len) // 2, (o_worst + p.match * o_len) // 2
    ia, io = pe.init(min1, min2)
    st = [ia[0], ia[1], io[0], io[1]]
    _, o_fw = pe.frame(p.policy, p.anchor, rc == 0)
    o_rc = 0 if o_fw else 1
    p1, p2 = pe.u32(g + base), pe.u32(g + 2 * base)
    row = lambda pos, da=0: (pos, pe.u32(pos + a_len - 1), sa - da, so, pe.u32(pos + 200), pe.u32(pos + 200 + o_len), rc, 0)
    if kind == "init":
        return st
    if kind in ("unpaired", "unpaired-other"):
        mate = p.anchor if kind == "unpaired" else 1 - p.anchor
        u = pe.aln(sa - 3, p1, a_len - 1, rc, mate, False)
        st[2 * mate] = u                                             # mate 1's in best_a, mate 2's in best_o
        return st
    if kind in ("pair", "other-anchor", "flipped-o"):
        a1, o1 = make_pair(p._replace(anchor=1 - p.anchor) if kind == "other-anchor" else p, row(p1))
        if kind == "flipped-o":
            o1 = o1[:3] + (1 - o1[3],) + o1[4:]
        return [a1, st[1], o1, st[3]]
    a1, o1 = make_pair(p, row(p1))
    delta = int(kind[3:]) if kind.startswith("two") else 2
    a2, o2 = make_pair(p, row(p2, delta))
    st = [a1, a2, o1, o2]
    if kind.startswith("two"):
        return st
    role, what = kind.split("-")[1][0], kind.split("-")[-1]
    mate, strand = (p.anchor, rc) if role == "a" else (1 - p.anchor, o_rc)
    if kind.startswith("vis"):
        slot = int(kind[-1])
        x = st[slot]
        st[slot] = (x[0], g, x[2], strand, mate, x[5])
        return st
    x = st[0]
    st[0] = (x[0], pe.u32(g + 1) if what == "pos" else g, x[2], 1 - strand if what == "rc" else strand, 1 - mate if what == "mate" else mate, x[5])
    for s in (1, 2, 3):                                              # no other slot may hold the locus
        if st[s][1] == g:
            st[s] = st[s][:1] + (pe.u32(g + 3),) + st[s][2:]
    return st


# ---- flatten lists ------------------------------------------------------------------------------------------------------------------
FlattenCfg = namedtuple("FlattenCfg", "policy anchor overlap min_frag max_frag genome_len scheme permissive uniform_pair")


def flatten_configs():
    """policy x anchor x overlap x min_frag x max_frag, the genome length, the scheme, the permissive tables and the uniform length pair
    rotating through them"""
    out = []
    for i, (policy, anchor, overlap, lo, hi) in enumerate(itertools.product(range(4), (0, 1), (0, 1), MIN_FRAGS, MAX_FRAGS)):
        k = i + i // 3 + i // 9
        out.append(FlattenCfg(policy, anchor, overlap, lo, hi, GENOMES[k % 3], ("e2e", "local")[i % 2], (i // 2) % 2 == 1, UNIFORM_PAIRS[(i // 4 + i // 9) % 4]))
    return out


def params_of(cfg, unpaired=1, max_effort=15, min_ext=30, max_ext=400):
    s = SCHEMES[cfg.scheme]
    return pe.Params(cfg.anchor, s.score_limit, pe.WORST_SCORE, s.match, s.txt_gap_open, s.txt_gap_ext, BAND, cfg.genome_len, cfg.policy, cfg.min_frag,
                     cfg.max_frag, cfg.overlap, unpaired, max_effort, min_ext, max_ext)


def loci(G):
    """the genome's start and end, the half band, loci that wrapped below zero, the two of the hand-worked rows, and ordinary ones"""
    out = [0, 1, BAND // 2, BAND // 2 + 1, 3, G - 1, G, G // 2, 400, 600] + [U32 - k for k in (0, 1, 5, 100, 400, 0xF)]
    if G < U32:
        out.append(G + 1)
    return out


# thresholds: min_score of the opposite job relative to o_opt = match * o_len -- one below, at, one above; then where max_text_gaps' loop
# turns once (0), four times (3) and pattern_len times (o_len - 1: reachable under the permissive tables alone)
THRESHOLDS = ("run", "opt-1", "opt", "opt+1", "gaps0", "gaps3", "gapscap")


def _anchor_score_for(p, st, thr, o_len, a_worst, o_worst):
    o_opt = p.match * o_len
    want = {"run": o_opt - 20, "opt-1": o_opt - 1, "opt": o_opt, "opt+1": o_opt + 1, "gaps0": o_opt + p.txt_gap_open,
            "gaps3": o_opt + p.txt_gap_open + 3 * p.txt_gap_ext, "gapscap": o_opt + p.txt_gap_open + o_len * p.txt_gap_ext}[thr]
    return pe.target_score(st, a_worst, o_worst) - (want - 1)        # min_score = target_pair - anchor_score + 1, where the clamps let it


def _finish(p, form, reads, hits, **more):
    return dict(p=p, form=form, a_len=tuple(r[0] for r in reads), o_len=tuple(r[1] for r in reads), min1=tuple(r[2] for r in reads),
                min2=tuple(r[3] for r in reads), best=tuple(tuple(r[4]) for r in reads), rid=tuple(h[0] for h in hits), seed=tuple(h[1] for h in hits),
                loc=tuple(h[2] for h in hits), score=tuple(h[3] for h in hits), **more)


def gapped_queue(n, seed):
    """a permutation of the hits with gaps (every seventh left out), its length no multiple of 64"""
    q = [int(v) for v in np.random.default_rng(seed).permutation(n) if v % 7 != 3]
    while len(q) % 64 == 0:
        q.pop()
    return tuple(q)


@functools.lru_cache(maxsize=None)
def flatten_list(cfg, form):
    """one read per hit: every locus x strand x (init, pair, two pairs); every threshold x strand x three length pairs; every state kind x strand"""
    p = params_of(cfg)
    s = SCHEMES[cfg.scheme]
    reads, hits = [], []

    def add(g, rc, kind, thr):
        k = len(reads)
        l1, l2 = pair_lengths(form, k, cfg.uniform_pair)
        m1, m2 = pair_tables(s, form, k, l1, l2, cfg.permissive if form == "uniform" else k % 5 == 4)
        a_len, o_len = (l2, l1) if cfg.anchor else (l1, l2)
        a_worst, o_worst = (m2, m1) if cfg.anchor else (m1, m2)
        st = make_state(kind, p, g, rc, a_len, o_len, m1, m2)
        reads.append((a_len, o_len, m1, m2, st))
        hits.append((k, seed_word(rc, k % 2), g, _anchor_score_for(p, st, thr, o_len, a_worst, o_worst)))

    for g, rc, kind in itertools.product(loci(cfg.genome_len), (0, 1), ("init", "pair", "two+2")):
        add(g, rc, kind, "run")
    for thr, rc, g in itertools.product(THRESHOLDS, (0, 1), (600, 601, 602, 603, 604, 605, 606, 607)):      # (eight pairs of lengths each, one or two of them permissive)
        add(g, rc, "init", thr)
    for kind, rc in itertools.product(STATE_KINDS, (0, 1)):
        add(600, rc, kind, "run")
        add(U32 - 5, rc, kind, "opt")
    return _finish(p, form, reads, hits, queue=gapped_queue(len(hits), 5))


@functools.lru_cache(maxsize=None)
def random_flatten_list(cfg, form, n_hits=20_000, n_reads=2_000):
    rng = np.random.default_rng(1234 + cfg.policy * 8 + cfg.anchor * 4 + (form == "ragged"))
    p = params_of(cfg)
    s = SCHEMES[cfg.scheme]
    pool = loci(cfg.genome_len)
    reads, hits = [], []
    for k in range(n_reads):
        l1, l2 = pair_lengths(form, k, cfg.uniform_pair)
        m1, m2 = pair_tables(s, form, k, l1, l2, cfg.permissive if form == "uniform" else k % 5 == 4)
        a_len, o_len = (l2, l1) if cfg.anchor else (l1, l2)
        g = int(pool[int(rng.integers(len(pool)))]) if rng.random() < 0.3 else int(rng.integers(0, 1 << 32))
        st = make_state(STATE_KINDS[int(rng.integers(len(STATE_KINDS)))], p, g, int(rng.integers(2)), a_len, o_len, m1, m2, base=int(rng.integers(1, 3000)))
        reads.append((a_len, o_len, m1, m2, st, g))
    for _ in range(n_hits):
        k = int(rng.integers(n_reads))
        a_len, o_len, m1, m2, st, g0 = reads[k]
        u = rng.random()
        g = g0 if u < 0.3 else int(st[int(rng.integers(4))][1]) if u < 0.5 else int(rng.integers(0, 1 << 32))
        hits.append((k, seed_word(int(rng.integers(2)), int(rng.integers(2))), g, int(rng.integers(min(m1, m2) - 40, p.match * a_len + 6))))
    return _finish(p, form, [r[:5] for r in reads], hits, queue=gapped_queue(n_hits, 6))


def roles(L, r):
    """(a_len, o_len, a_worst, o_worst, o_opt) of read r: the tables by mate become scores by role here, as the header says"""
    p = L["p"]
    a_worst, o_worst = (L["min2"][r], L["min1"][r]) if p.anchor else (L["min1"][r], L["min2"][r])
    return L["a_len"][r], L["o_len"][r], a_worst, o_worst, p.match * L["o_len"][r]


def want_anchor_flatten(L):
    """-> rows (read_id, flags, win_begin, win_end, min_score) of every hit"""
    out = []
    for r, seed, g in zip(L["rid"], L["seed"], L["loc"]):
        a_len, o_len, a_worst, o_worst, o_opt = roles(L, r)
        out.append((r,) + pe.anchor_flatten(L["p"], list(L["best"][r]), (seed >> 13) & 1, g, a_len, a_worst, o_worst, o_opt))
    return out


def want_opposite_flatten(L):
    """-> rows (read_id, flags, win_begin, win_end, min_score, reason, gaps) of every queue slot"""
    p = L["p"]
    out = []
    for i in L["queue"]:
        r, rc, g = L["rid"][i], (L["seed"][i] >> 13) & 1, L["loc"][i]
        a_len, o_len, a_worst, o_worst, o_opt = roles(L, r)
        row = pe.opposite_flatten(p, list(L["best"][r]), rc, g, L["score"][i], a_len, o_len, a_worst, o_worst, o_opt)
        out.append((r,) + row + (pe.max_text_gaps(p.match, p.txt_gap_open, p.txt_gap_ext, row[3], o_len),))
    return out


# ---- output lists -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def anchor_output_list(scheme_name):
    """score in { min - 1, min, min + 1, worst, worst + 1, NVBIO_SCORE_MIN } x min_score in { a real value, score_limit, INT32_MAX } x sink.x in
    { 0, 1, 0xFFFFFFFF } x a window begin that makes the sum wrap or not -> (scores, sink_x, win_begin, min_scores, worst_score)"""
    s = SCHEMES[scheme_name]
    real = min_score(s, 100) + 5
    rows = []
    for ms in (real, s.score_limit, pe.INT32_MAX, pe.WORST_SCORE, pe.WORST_SCORE + 1):
        for score in (ms - 1, ms, min(ms + 1, pe.INT32_MAX), pe.WORST_SCORE, pe.WORST_SCORE + 1, pe.SCORE_MIN):
            for sx, wb in itertools.product((0, 1, U32), (0, 5000, U32, U32 - 1)):
                rows.append((pe.i32(score), sx, wb, ms))
    return tuple(zip(*rows)) + (pe.WORST_SCORE,)


@functools.lru_cache(maxsize=None)
def opposite_output_list(scheme_name):
    """jobs that ran, that did not (we == wb, and we < wb as data) with a stale passing score, sinks of 0xFFFFFFFF, over a queue with gaps into a
    hit array longer than the queue -> (queue, n_hits, scores, sink_x, win_begin, win_end, min_scores, worst_score)"""
    s = SCHEMES[scheme_name]
    real = min_score(s, 150) + 3
    rows = []
    for (wb, we), ms in itertools.product(((100, 400), (0, 0), (700, 700), (900, 100), (0, 1), (U32 - 10, U32), (U32, 0)), (real, s.score_limit, real + 40)):
        for score, sx in itertools.product((ms - 1, ms, ms + 1, ms + 30, pe.WORST_SCORE, pe.SCORE_MIN), (0, 7, U32, U32 - 1)):
            rows.append((pe.i32(score), sx, wb, we, ms))
    n_hits = 2 * len(rows) + 5
    queue = tuple(int(v) for v in np.random.default_rng(77).permutation(n_hits)[:len(rows)])
    assert len(rows) % 64 != 0
    return (queue, n_hits) + tuple(zip(*rows)) + (pe.WORST_SCORE,)


# ---- reduce lists -------------------------------------------------------------------------------------------------------------------
ReduceCfg = namedtuple("ReduceCfg", "policy anchor unpaired ext uniform_pair")
MAX_EFFORT, MIN_EXT, MAX_EXT = 3, 30, 40
EXTS = (0, MIN_EXT - 1, MIN_EXT, MAX_EXT - 1, MAX_EXT)
TRYS = (0, 1, 2, MAX_EFFORT)
REDUCE_STATES = ("init", "unpaired", "unpaired-other", "pair", "other-anchor", "flipped-o", "two+0", "two+1", "two+3", "two+400", "two-1", "low-pair")
HIT_COUNTS = (0, 1, 2, 3, 65, 300)


def reduce_configs():
    return [ReduceCfg(policy, anchor, unpaired, ext, UNIFORM_PAIRS[(i // 3) % 4])
            for i, (policy, anchor, unpaired, ext) in enumerate(itertools.product(range(4), (0, 1), (0, 1), EXTS))]


def _row_of_pair(a, o, top=0):
    """the hit row score_reduce_paired would turn into the pair (a, o)"""
    return (a[1], pe.u32(a[1] + a[2]), a[0], o[0], o[1], pe.u32(o[1] + o[2]), a[3], top)


def _single_rows(p, st, a_len, o_len):
    """hit rows that force every branch against state st: (label, row)"""
    dist = a_len // 2
    a1, a2, o1, o2 = st
    best, second = pe.best_score(st), pe.second_score(st)
    far = 1_000_000
    rows = []
    paired = pe.is_paired(a1)
    if paired:
        held = _row_of_pair(a1, o1) if a1[4] == p.anchor else _row_of_pair(o1, a1)
        rows.append(("same-as-first", held))
        if pe.is_paired(a2):
            rows.append(("same-as-second", _row_of_pair(a2, o2) if a2[4] == p.anchor else _row_of_pair(o2, a2)))
        gx, gy, s1, s2, ox, oy, rc, _ = held
        mid = (best + second) // 2 if best - second > 1 else second + 1
        sc = lambda total: (total - s2, s2)
        rows.append(("better", (far, far + a_len, s1 + 1, s2, far + 300, far + 300 + o_len, rc, 0)))
        rows.append(("equal-best", (far, far + a_len, s1, s2, far + 300, far + 300 + o_len, rc, 1)))
        rows.append(("equal-second", (far, far + a_len) + sc(second) + (far + 300, far + 300 + o_len, rc, 0)))
        rows.append(("between-far", (far, far + a_len) + sc(mid) + (far + 300, far + 300 + o_len, rc, 1)))
        rows.append(("below", (far, far + a_len) + sc(second - 1) + (far + 300, far + 300 + o_len, rc, 0)))
        # the distinctness rule at its distance: the END positions (sink, opposite sink) dist and dist + 1 from the best pair's, on either mate
        steps = (-dist - 1, -dist, 0, dist, dist + 1)
        for ia, io in itertools.product(range(5), repeat=2):
            if (ia, io) != (2, 2) and (ia == 2 or io == 2 or abs(ia - 2) == abs(io - 2)):
                rows.append(("near-%d-%d" % (ia, io), (gx, pe.u32(gy + steps[ia])) + sc(mid) + (ox, pe.u32(oy + steps[io]), rc, (ia + io) & 1)))
        rows.append(("other-strand", (gx, gy) + sc(mid) + (ox, oy, 1 - rc, 0)))
    m1 = a1 if p.anchor == a1[4] else o1
    m2 = a2 if p.anchor == a2[4] else o2
    rc = m1[3] if m1[1] != pe.NONE else 0
    lo = m2[0] - 50
    worst = pe.WORST_SCORE
    pos = m1[1] if m1[1] != pe.NONE else 5000
    for top in (0, 1):
        rows.append(("mate-better", (far, far + a_len, m1[0] + 1, worst, 0, 0, rc, top)))
        rows.append(("mate-equal", (far, far + a_len, m1[0], worst, 0, 0, rc, top)))
        rows.append(("mate-second-far", (far, far + a_len, m2[0] + 1, worst, 0, 0, rc, top)))
        rows.append(("mate-low", (far, far + a_len, lo, worst, 0, 0, rc, top)))
    for i, d in enumerate((-dist - 1, -dist, dist, dist + 1)):
        rows.append(("mate-second-near-%d" % i, (pe.u32(pos - d), pe.u32(pos - d + a_len), m2[0] + 1, worst, 0, 0, rc, 0)))
    rows.append(("mate-second-strand", (pos, pe.u32(pos + a_len), m2[0] + 1, worst, 0, 0, 1 - rc, 1)))
    return rows


@functools.lru_cache(maxsize=None)
def reduce_list(cfg, form):
    """reads: every state x every single row; the failure grid (trys x top_flag); the two-hit orders; hit lists of HIT_COUNTS.  Every third read is
    NOT active (its state, trys and sizes must stay); active[] entries carry bit 31 on odd slots; hits_first is not contiguous (rows of inactive
    reads lie between, and the reads are visited in a permuted order)"""
    fc = FlattenCfg(cfg.policy, cfg.anchor, 1, 0, 500, U32, "e2e", False, cfg.uniform_pair)
    p = params_of(fc, cfg.unpaired, MAX_EFFORT, MIN_EXT, MAX_EXT)
    s = SCHEMES["e2e"]
    rng = np.random.default_rng(99 + cfg.policy)
    reads, lists = [], []

    def new_read(kind, g=50_000):
        k = len(reads)
        l1, l2 = pair_lengths(form, k, cfg.uniform_pair)
        m1, m2 = pair_tables(s, form, k, l1, l2, False)
        a_len, o_len = (l2, l1) if cfg.anchor else (l1, l2)
        if kind == "low-pair":                                       # a pair whose end positions lie below dist: the clamp at pos < dist
            st = make_state("pair", p, 0, k % 2, a_len, o_len, m1, m2, base=0)
            a1, o1 = st[0], st[2]
            st = [a1[:2] + (a_len // 4,) + a1[3:], st[1], (o1[0], 0, max(a_len // 2 - 1, 0)) + o1[3:], st[3]]
        else:
            st = make_state(kind, p, g, k % 2, a_len, o_len, m1, m2)
        return (a_len, o_len, m1, m2, st)

    def add(read, rows, trys):
        reads.append(read)
        lists.append((tuple(rows), trys))

    n = 0
    for kind in REDUCE_STATES:
        probe = new_read(kind)
        for label, _ in _single_rows(p, probe[4], probe[0], probe[1]):
            read = new_read(kind)
            row = dict(_single_rows(p, read[4], read[0], read[1]))[label]
            add(read, [row], TRYS[(n + n // 4) % 4])
            n += 1
    for kind, trys, top in itertools.product(("init", "pair", "two+3"), TRYS, (0, 1)):            # the failure grid
        read = new_read(kind)
        row = dict(_single_rows(p, read[4], read[0], read[1]))["mate-low"]
        add(read, [row[:7] + (top,)], trys)
    for order in ("ub-ub", "ub-pair", "pair-ub", "second-best", "ub-us-fail"):                       # the two-hit orders
        kind = "two+400" if order == "second-best" else "init"
        read = new_read(kind)
        a_len, o_len, m1, m2, st = read
        a_w = m2 if cfg.anchor else m1
        up = lambda pos, sc: (pos, pos + a_len, sc, pe.WORST_SCORE, 0, 0, 0, 0)
        pr = lambda pos, sa, so: (pos, pos + a_len, sa, so, pos + 300, pos + 300 + o_len, 0, 0)
        if order == "ub-ub":                                         # the second is lower than the first, above the initial: the local copy decides
            rows = [up(1000, a_w + 9), up(9000, a_w + 4), up(20000, a_w + 6)]
        elif order == "ub-pair":
            rows = [up(1000, a_w + 9), pr(9000, max(m1, m2) + 8, -3)]        # above the initial state whichever mate's score it holds
        elif order == "pair-ub":
            rows = [pr(9000, max(m1, m2) + 8, -3), up(1000, a_w + 9)]
        elif order == "second-best":
            b = pe.best_score(st)
            rows = [pr(900_000, b - 40, 0), pr(800_000, b + 5, 0), pr(700_000, b - 2, 0)]
        else:
            rows = [up(1000, a_w + 9), up(1000 + a_len // 2, a_w + 5), up(3000, a_w + 5), up(1000, a_w - 1), up(1000, a_w - 2)]
        add(read, rows, 2)
    for count, kind in itertools.product(HIT_COUNTS, ("init", "pair")):                              # hit lists of every length
        read = new_read(kind)
        a_len, o_len, m1, m2, st = read
        base = pe.best_score(st) if pe.is_paired(st[0]) else (m1 + m2)
        rows = []
        for _ in range(count):
            pos = int(rng.integers(0, 40)) * (a_len // 2 + 1) + 100
            total = base + int(rng.integers(-6, 4))
            so = int(rng.integers(-4, 1))
            rows.append((pos, pos + a_len, total - so, so, pos + 250, pos + 250 + o_len, int(rng.integers(2)), int(rng.integers(2))) if rng.random() < 0.6
                        else (pos, pos + a_len, (m2 if cfg.anchor else m1) + int(rng.integers(-3, 8)), pe.WORST_SCORE, 0, 0, int(rng.integers(2)), int(rng.integers(2))))
        add(read, rows, TRYS[count % 4])
    # the hit arrays: every read's rows, in a permuted order of reads; every third read inactive
    R = len(reads)
    order = [int(v) for v in rng.permutation(R)]
    first_of, rows_all = {}, []
    for r in order:
        first_of[r] = len(rows_all)
        rows_all.extend(lists[r][0])
        rows_all.append((0, 0, 0, 0, 0, 0, 0, 0))                    # a slot no read owns
    act = [r for r in range(R) if r % 3 != 2]
    active = tuple(r | ((1 << 31) if t % 2 else 0) for t, r in enumerate(act))
    return dict(p=p, form=form, ext=cfg.ext, a_len=tuple(r[0] for r in reads), o_len=tuple(r[1] for r in reads), min1=tuple(r[2] for r in reads),
                min2=tuple(r[3] for r in reads), best=tuple(tuple(r[4]) for r in reads), trys=tuple(l[1] for l in lists), rows=tuple(rows_all),
                active=active, first=tuple(first_of[r] for r in act), count=tuple(len(lists[r][0]) for r in act))


def want_reduce(L, n_active=None):
    """-> ({read: (best_a, best_o, trys, erased)}, branches of every hit of every active read) over the first n_active slots"""
    out, branches = {}, []
    for t in range(len(L["active"]) if n_active is None else n_active):
        r = L["active"][t] & 0x7FFFFFFF
        rows = L["rows"][L["first"][t]:L["first"][t] + L["count"][t]]
        ba, bo, trys, erased, br = pe.reduce_read(L["p"], list(L["best"][r]), L["trys"][r], rows, L["a_len"][r], L["ext"])
        out[r] = (ba, bo, trys, erased)
        branches.append(br)
    return out, branches


# ---- numpy forms (what the device sees) ---------------------------------------------------------------------------------------------
def best_arrays(best):
    """states -> (best_a, best_o) int64 [R, 2, 4] holding uint32 bit patterns / signed scores as Python integers"""
    word = lambda a: (a[0], a[1], a[2], pe.flags_word(a))
    ba = np.array([[word(b[0]), word(b[1])] for b in best], dtype=np.int64).reshape(-1, 2, 4)
    bo = np.array([[word(b[2]), word(b[3])] for b in best], dtype=np.int64).reshape(-1, 2, 4)
    return ba, bo


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.array(lengths, dtype=np.int64))]).astype(np.uint32)
