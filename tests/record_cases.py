"""The planted case lists of the record-format edge tests (test_record_cases_oracle.py proves on the CPU that each list reaches what it
is for, test_gpu_record_edges.py runs the SAM and BAM kernels over them): refs / records dicts in the shape sam_cpu and bam_cpu take.
Nothing here is drawn at random: every record is placed by a rule stated where it is made, reads and qualities are arithmetic patterns,
and every list is built once per process and never modified.

    genome_refs, many_refs(k), one_long_ref     reference tables: starts past 2^31, a binary search over 1 ... 1025 entries, 10-digit POS
    coordinate_records(key, paired)             records at the first / last base of every sequence, on and across every reg2bin level, far mates
    class_shapes(fmt), class_batch(fmt, shape)  one declared shape per LDS class of sam_plan / bam_plan and the pairs on each class boundary
    too_long_batch(fmt, which)                  maxima declared below what two records really have: NVBIO_*_STATUS_TOO_LONG
    cut_md_batch(fmt, stride)                   MDS streams that end inside a token
    BGZF_SIZES, SCAN_N, scan_batch_41           payloads over every byte shift of the framing kernel; the record count of the scan's second round

The two host formulas are restated here (sam_need, bam_need) from the headers of csrc/sam.hip and csrc/bam.hip:
    need = 16 + bound + stage, the class is the smallest of SAM_CLASSES / BAM_CLASSES that holds it, cap = class - stage."""
import functools

import numpy as np

import bam_cpu
import sam_cpu

M_, I_, D_, S_ = 0, 1, 2, 3
ALIGNED, RC, READ_2, PAIRED = 1, 2, 4, 8
SAM_CLASSES = (1024, 2048, 4096, 8192, 16384)
BAM_CLASSES = (512, 1024, 2048, 4096, 8192, 16384)
BAM_GROUPS = {512: 16, 1024: 16, 2048: 16, 4096: 16, 8192: 8, 16384: 4}      # records to a workgroup; SAM: 4 everywhere
LEVELS = (14, 17, 20, 23, 26, 29)                                    # reg2bin: a bin of level s spans 2^s bases


# ---- the host formulas --------------------------------------------------------------------------------------------------------------
def _stage(ms):
    return (ms + 15) & ~15 if ms else 0


def sam_need(name, ref_name, cs, mrl, ms):
    md = 2 * ms + 16 if ms else 1
    return 16 + (name + 2 * ref_name + 2 * mrl + 6 * cs + md + 192) + _stage(ms)


def bam_need(name, cs, mrl, ms):
    md = 2 * ms + 16 if ms else 0
    return 16 + (name + 4 * cs + mrl + (mrl + 1) // 2 + md + 72) + _stage(ms)


def need_of(fmt, shape):
    if fmt == "sam":
        return sam_need(shape["name"], shape["ref_name"], shape["cs"], shape["mrl"], shape["ms"])
    return bam_need(shape["name"], shape["cs"], shape["mrl"], shape["ms"])


def class_of(fmt, need):
    """the LDS class the host picks, 0 when none holds `need` (NVBIO_ERR_UNSUPPORTED)"""
    return next((c for c in (SAM_CLASSES if fmt == "sam" else BAM_CLASSES) if need <= c), 0)


def record_bytes(fmt, refs, rec, i, flags=0):
    p = sam_cpu.sam_record(refs, rec, i) if fmt == "sam" else bam_cpu.bam_record(refs, rec, i, flags)
    return 0 if p is None else len(p)


# ---- records from explicit specifications ------------------------------------------------------------------------------------------
def _name(i, length):
    """printable, no tab: 33 ... 126"""
    return bytes(33 + (i * 7 + k * 13 + (k >> 4)) % 94 for k in range(length))


class Batch:
    """records added one by one; build() lays them out as sam_cpu's dict"""

    def __init__(self):
        self.specs = []

    def add(self, rlen, pos=0, els=None, name_len=None, state=0, mds=None, mds_len=None):
        """els: the CIGAR (last element first, as a traceback writes it), None for an unaligned read; mds: the MDS bytes, mds_len: what
        mds_lens says (default: their count).  Every third record is reverse-complemented."""
        i = len(self.specs)
        st = state | (ALIGNED if els is not None else 0) | (RC if i % 3 == 1 else 0)
        self.specs.append(dict(rlen=rlen, pos=pos, els=els or [], name_len=(i * 5) % 23 + 1 if name_len is None else name_len, state=st,
                               mds=list(mds or []), mds_len=mds_len))
        return i

    def build(self, cigar_stride, mds_stride=None, paired=False, quals=True):
        sp, n = self.specs, len(self.specs)
        assert not paired or n % 2 == 0
        read_index = np.concatenate([[0], np.cumsum([s["rlen"] for s in sp])]).astype(np.uint32)
        t = np.arange(int(read_index[-1]), dtype=np.uint64)
        v = ((t * np.uint64(2654435761)) >> np.uint64(13)) % np.uint64(23)
        reads = np.where(v < 20, v % np.uint64(4), np.where(v < 22, 4, 15)).astype(np.uint8)      # about 9% N, 4% another code that prints N
        cigars = np.zeros((n, cigar_stride), np.uint16)
        cigar_lens = np.zeros(n, np.uint32)
        mds = None if mds_stride is None else np.zeros((n, mds_stride), np.uint8)
        mds_lens = None if mds_stride is None else np.zeros(n, np.uint32)
        for i, s in enumerate(sp):
            assert len(s["els"]) <= cigar_stride and all(0 <= l < 16384 for l, _ in s["els"])
            cigars[i, :len(s["els"])] = [l << 2 | o for l, o in s["els"]]
            cigar_lens[i] = len(s["els"])
            if mds is not None:
                m = s["mds"][:mds_stride]
                mds[i, :len(m)] = m
                mds_lens[i] = len(s["mds"]) if s["mds_len"] is None else s["mds_len"]
        k = np.arange(n, dtype=np.int64)
        return dict(names=[_name(i, s["name_len"]) for i, s in enumerate(sp)], reads=reads, read_index=read_index,
                    quals=(((t * np.uint64(40503)) >> np.uint64(5)) % np.uint64(94)).astype(np.uint8) if quals else None,
                    state=np.array([s["state"] for s in sp], np.uint8), pos=np.array([s["pos"] for s in sp], np.uint32),
                    score=(-(k * 37 % 2000)).astype(np.int32), second_score=np.where(k % 2 == 1, sam_cpu.SCORE_MIN, -(k * 53 % 3000)).astype(np.int32),
                    ed=(k * 7 % 300).astype(np.uint32), mapq=(k * 11 % 256).astype(np.uint8), cigars=cigars, cigar_lens=cigar_lens, mds=mds,
                    mds_lens=mds_lens, mate_of=(np.arange(n, dtype=np.uint32) ^ 1) if paired else None, reads_reversed=True)


def mds_stream(tokens):
    body = [b for t in tokens for b in t]
    n = len(body) + 2
    return [n & 255, n >> 8] + body


# ---- reference tables --------------------------------------------------------------------------------------------------------------
def _refs(lengths, name_lens):
    si = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])
    assert si[-1] < 1 << 32
    return dict(sequence_index=si.astype(np.uint32), names=[bytes(65 + (s * 3 + k * 7) % 26 for k in range(l)) for s, l in enumerate(name_lens)])


@functools.lru_cache(None)
def genome_refs():
    """ten sequences, 2,760,864,386 bases (below the index's 0xC0000000): five of 2^29, one of 1 base, one of 2^26; sequences 7, 8 and 9
    start past 2^31; names of 1 ... 100 bytes, 63 / 64 / 65 among them"""
    return _refs([1 << 29, 1, 1 << 29, 1 << 26, 1 << 29, 1000003, 1 << 29, 1 << 29, (1 << 23) + 5, 12345], [1, 100, 64, 65, 63, 16, 4, 33, 2, 80])


@functools.lru_cache(None)
def many_refs(k):
    """k sequences of 50 ... 150 bases, no two neighbours equal"""
    return _refs([50 + (j * 37) % 101 for j in range(k)], [1 + j % 9 for j in range(k)])


@functools.lru_cache(None)
def one_long_ref():
    return _refs([3100000000], [7])


# ---- coordinates -------------------------------------------------------------------------------------------------------------------
def _placements(refs):
    """(what, genome position, CIGAR) of every planted alignment, and the far pairs [(a, b)] as indices into that list"""
    si = refs["sequence_index"].astype(np.int64)
    k = len(refs["names"])
    out, far = [], []
    for s in range(k):
        b, L = int(si[s]), int(si[s + 1] - si[s])
        out.append(("first", b, [(min(L, 7), M_)]))
        out.append(("last", b + L - 1, [(1, M_)]))
        if k <= 64 or s in (0, 1, k // 2, k - 2, k - 1):
            r = min(L, 9)
            els = [(2, M_), (2, D_), (r - 4, M_)] if r >= 5 else [(r, M_)]          # r reference bases
            out.append(("ends with", b + L - r, els))
            out.append(("one past", b + L - r + 1, els))                               # bridges (or runs past the genome)
    q = max(range(k), key=lambda s: (int(si[s + 1] - si[s]), int(si[s])))              # the longest sequence, the last of them
    b, L = int(si[q]), int(si[q + 1] - si[q])
    for s in LEVELS:
        if L < 1 << s:
            continue
        for m in sorted({1, ((L >> s) - 1) | 1}):                                      # odd multiples: the crossing interval belongs one level up
            B = m << s
            out.append(("ends on 2^%d" % s, b + B - 10, [(10, M_)]))
            out.append(("crosses 2^%d from below" % s, b + B - 9, [(10, M_)]))
            out.append(("crosses 2^%d from above" % s, b + B - 1, [(10, M_)]))
    for w in range(1, 11):                                                             # POS = 10^(w - 1) and 10^w - 1
        for own in (10 ** (w - 1) - 1, 10 ** w - 2):
            if own + 5 <= L:
                out.append(("POS of %d digits" % w, b + own, [(5, M_)]))
    spans = [L] + [t for t in (99999999, 100000000, 1 << 28, (1 << 31) - 1, (1 << 31) + 1, 3000000000) if t + 1000 <= L]
    for t in spans:                                                                    # TLEN = t: the first at own 0 (or 1000), the second ends t behind
        a0 = 0 if t == L else 1000
        out.append(("far first", b + a0, [(10, M_)] if L >= 10 else [(1, M_)]))
        out.append(("far second", b + a0 + t - 1, [(1, M_)]))
        far.append((len(out) - 2, len(out) - 1))
    return out, far


@functools.lru_cache(None)
def coordinate_records(refs_key, paired=False):
    """refs_key: "genome", "long" or k (many_refs).  Single-end: one record per placement.  Paired: every placement is one mate of a pair
    whose other mate goes, by turns, 40 bases behind it, 40 bases before it, to the next sequence, unaligned, and one base past the end of
    the sequence (written as unmapped: the anchor then prints the mate as it would any other); the far pairs come in both orders.
    -> (refs, rec, labels) with labels[i] what record i is there for"""
    refs = refs_of(refs_key)
    si = refs["sequence_index"].astype(np.int64)
    k = len(refs["names"])
    places, far = _placements(refs)
    b, labels = Batch(), []
    md = lambda j, rlen: mds_stream([[0, rlen]]) if j % 2 == 0 else []
    read_len = lambda els: sum(l for l, t in els if t != D_)
    if not paired:
        for j, (what, pos, els) in enumerate(places):
            b.add(read_len(els), pos, els, mds=md(j, read_len(els)))
            labels.append(what)
        return refs, b.build(4, 16), labels
    in_far = {i for pair in far for i in pair}
    for j, (what, pos, els) in enumerate(places):
        if j in in_far:
            continue
        s = sam_cpu.sequence_of(refs, pos)
        lo, L = int(si[s]), int(si[s + 1] - si[s])
        mate_els, rule = [(min(L, 3), M_)], j % 5
        if rule == 0:
            mate = (min(pos + 40, lo + L - min(L, 3)), mate_els)
        elif rule == 1:
            mate = (max(pos - 40, lo), mate_els)
        elif rule == 2:
            mate = (int(si[(s + 1) % k]), [(1, M_)])
        elif rule == 3:
            mate = None
        else:
            mate = (lo + L - min(L, 3) + 1, mate_els)
        pair = [(what, pos, els), ("mate, rule %d" % rule,) + (mate if mate else (0, None))]
        flag = PAIRED if j % 2 else 0
        for h, (w, p, e) in enumerate(pair if j % 3 else pair[::-1]):                  # the anchor is the second record of every third pair
            b.add(read_len(e) if e else 4, p, e, state=flag | (READ_2 if h else 0), mds=md(j + h, read_len(e) if e else 4))
            labels.append(w)
    for a, c in far:
        for order in ((a, c), (c, a)):
            for h, i in enumerate(order):
                what, pos, els = places[i]
                b.add(read_len(els), pos, els, state=PAIRED | (READ_2 if h else 0), mds=md(h, read_len(els)))
                labels.append(what)
    return refs, b.build(4, 16, paired=True), labels


def refs_of(key):
    return genome_refs() if key == "genome" else one_long_ref() if key == "long" else many_refs(key)


# ---- LDS classes -------------------------------------------------------------------------------------------------------------------
# one declared shape inside every class (name, ref name, cigar_stride, max_read_len, mds_stride)
_BASE = {"bam": {512: (20, 5, 4, 100, None), 1024: (40, 5, 8, 300, None), 2048: (40, 5, 100, 200, 64), 4096: (254, 16, 500, 300, 64),
                 8192: (40, 16, 1024, 300, 320), 16384: (40, 16, 3000, 300, 320)},
         "sam": {1024: (20, 5, 4, 100, None), 2048: (40, 16, 8, 300, 64), 4096: (254, 16, 300, 300, 64), 8192: (40, 16, 700, 300, 320),
                 16384: (40, 16, 2000, 300, 320)}}


def _shape(fmt, name, ref_name, cs, mrl, ms, what):
    s = dict(name=name, ref_name=ref_name, cs=cs, mrl=mrl, ms=ms, what=what)
    s["need"] = need_of(fmt, s)
    s["cls"] = class_of(fmt, s["need"])
    return s


def _solve(fmt, base, target):
    """the base shape with max_name_len (40 ... 45) and cigar_stride moved so that need == target"""
    name, ref_name, cs, mrl, ms = base
    per = 6 if fmt == "sam" else 4
    rest = target - need_of(fmt, dict(name=0, ref_name=ref_name, cs=0, mrl=mrl, ms=ms))
    name = 40 + (rest - 40) % per
    assert rest - name > 0
    return name, ref_name, (rest - name) // per, mrl, ms


@functools.lru_cache(None)
def class_shapes(fmt):
    """per class C: the base shape, the shape with need == C (the last one in), the shape with need == C + 1 (the first one in the next
    class; past the largest class: refused, cls == 0)"""
    out = []
    for c, base in _BASE[fmt].items():
        out.append(_shape(fmt, *base, what="inside %d" % c))
        out.append(_shape(fmt, *_solve(fmt, base, c), what="need == %d" % c))
        out.append(_shape(fmt, *_solve(fmt, base, c + 1), what="need == %d + 1" % c))
    return out


def shape_id(shape):
    return shape["what"].replace(" ", "")


@functools.lru_cache(None)
def class_refs(ref_name_len):
    """two sequences of 2^29 bases: a name of ref_name_len bytes and one of 1"""
    return _refs([1 << 29, 1 << 29], [ref_name_len, 1])


D_LENS = (3, 45, 678, 9012, 16383)                                    # widths 1 ... 5


def full_cigar(cs, rlen, widest=False):
    """exactly cs elements over a read of rlen: min(rlen, cs / 2) elements that consume the read (M I S by turns) between deletions of 1 ... 5
    digits; widest: one M of the whole read and cs - 1 deletions of 5 digits, the most text cs elements can print"""
    if widest:
        return [(rlen, M_)] + [(16383 - e % 6000, D_) for e in range(cs - 1)]
    n_read = max(1, min(rlen, cs // 2))
    parts = [rlen // n_read + (1 if e < rlen % n_read else 0) for e in range(n_read)]
    els, d = [], 0
    for e in range(cs):
        if parts and (e % 2 == 0 or cs - e <= len(parts)):
            els.append((parts.pop(), (M_, I_, M_, S_)[e // 2 % 4]))
        else:
            els.append((D_LENS[d % 5], D_))
            d += 1
    assert not parts and len(els) == cs
    return els


def dense_mds(ms):
    """the well-formed stream of at most ms bytes that prints the most: match runs do not print next to each other (they merge into one
    number), a mismatch prints 1 character from 2 bytes, a deletion of l prints l + 2 from l + 2, so the densest is [0, 255] [3, 1, c]
    by turns: 6 characters from 5 bytes, 1.2 a byte -- below the 1.5 (a lone [0, 255]) the bound allows for"""
    tokens = []
    while 2 + sum(len(t) for t in tokens) + 5 <= ms:
        tokens += [[0, 255], [3, 1, len(tokens) % 4]]
    if 2 + sum(len(t) for t in tokens) + 2 <= ms:
        tokens.append([0, 255])
    return mds_stream(tokens)


NEAR, TUNER = 21, 20                                                   # the record at the bound and the one before it, whose name sets the residue
BATCH_SIZES = (33, 70, 37, 49, 53)                                     # each leaves a short last workgroup of 4, 8 and 16 records


def _bumpable(j):
    """the records whose names may grow by up to 15 bytes to move the offsets behind them: the short-CIGAR ones.  Record 22 (LONG_B of the
    TOO_LONG batches, whose length is set to the byte) is left alone in the class batches too, so that both kinds of batch share one rule"""
    return j not in (TUNER, NEAR, NEAR + 1) and j % 7 != 3 and j % 5 != 0


def _class_specs(shape, n, b, tuner_name, bump):
    """the n records of a class batch but the NEAR one, which the caller adds in its place; bump: {record: bytes added to its name}"""
    name, cs, mrl, ms = shape["name"], shape["cs"], shape["mrl"], shape["ms"]
    half = 1 << 29
    for j in range(n):
        pos = (j % 2) * half + 1000 + j * 1000003
        rlen = mrl if j % 4 == 1 else (j * 37) % mrl + 1
        md = None if ms is None else [[], mds_stream([[0, min(rlen, 255)]]), dense_mds(ms), mds_stream([[0, 9], [1, 2], [3, 2, 0, 3], [2, 1, 1], [0, 1]])][j % 4]
        if j == TUNER:
            b.add(5, name_len=tuner_name)
        elif j == NEAR:
            yield j
        elif j % 7 == 3:
            b.add(rlen, name_len=name)                                                 # unaligned, the longest name
        elif j % 5 == 0:
            b.add(rlen, pos, full_cigar(cs, rlen), name_len=name if j % 10 == 0 else None, mds=md)
        else:
            few = [(rlen, M_)] if cs < 3 or rlen < 3 else [(1, S_), (j + 1, D_), (rlen - 1, M_)]
            b.add(rlen, pos, few, name_len=min(name - 15, (j * 5) % 23 + 1) + bump.get(j, 0), mds=md)


def _spread(fmt, refs, build, n, target, residue):
    """names grown so that the records start at every residue mod 16 and record `target` at `residue`: the bumpable records before the TUNER
    and behind `target` each move the next offset to a residue not seen yet, the TUNER sets the target's -> (tuner name, bump)"""
    rec = build(1, {})
    lens = [record_bytes(fmt, refs, rec, i) for i in range(n)]
    bump, seen, off = {}, set(), 0
    for j in range(n):
        if j == TUNER:
            tuner = 1 + (residue - (off + sum(lens[TUNER:target]))) % 16
            lens[j] += tuner - 1
        seen.add(off % 16)
        if _bumpable(j) and not TUNER <= j <= target and j + 1 != TUNER:
            want = [x for x in range(16) if (off + lens[j] + x) % 16 not in seen]
            bump[j] = want[0] if want else 0
            lens[j] += bump[j]
        off += lens[j]
    return tuner, bump


@functools.lru_cache(None)
def class_batch(fmt, shape_index):
    """-> (refs, rec, shape): 33 ... 70 records whose arrays have the shape's strides and whose longest name and read are the shape's;
    every fifth has cigar_lens == cigar_stride; record NEAR has the longest name, the longest read, the widest full CIGAR, XS and the densest
    MD, and starts at 15 mod 16"""
    shape = class_shapes(fmt)[shape_index]
    refs = class_refs(shape["ref_name"])
    n = BATCH_SIZES[shape_index % len(BATCH_SIZES)]

    def build(tuner_name, bump):
        b = Batch()
        for j in _class_specs(shape, n, b, tuner_name, bump):
            b.add(shape["mrl"], 12345, full_cigar(shape["cs"], shape["mrl"], widest=True), name_len=shape["name"],
                  mds=None if shape["ms"] is None else dense_mds(shape["ms"]))
        rec = b.build(shape["cs"], shape["ms"])
        rec["second_score"][NEAR], rec["score"][NEAR], rec["ed"][NEAR] = -65536, -65536, 300
        return rec

    return refs, build(*_spread(fmt, refs, build, n, NEAR, 15)), shape


# ---- TOO_LONG ----------------------------------------------------------------------------------------------------------------------
LONG_A, LONG_B = NEAR, NEAR + 1                                                # in the middle of a workgroup of 4 (20 ... 23), 8 (16 ... 23) and 16 (16 ... 31)


@functools.lru_cache(None)
def too_long_batch(fmt, which):
    """which: "smallest" (the base shape of the smallest class) or "largest" (the shape with need == 16384).  Records LONG_A and LONG_B have
    reads and names longer than the shape declares: LONG_A overflows by hundreds of bytes; LONG_B has cap - 3 bytes and starts at 9 mod 16,
    so it fits a group's LDS by its length alone and not from where it starts.  -> (refs, rec, shape, cap)"""
    shapes = class_shapes(fmt)
    shape = shapes[0] if which == "smallest" else shapes[-2]
    assert shape["cls"] == ((SAM_CLASSES if fmt == "sam" else BAM_CLASSES)[0 if which == "smallest" else -1])
    refs = class_refs(shape["ref_name"])
    cap = shape["cls"] - _stage(shape["ms"])
    cs, ms = shape["cs"], shape["ms"]
    md = None if ms is None else dense_mds(ms)

    def build(tuner_name, bump, b_name=1, b_read=shape["mrl"] + 1):
        b = Batch()
        for j in _class_specs(shape, 37, b, tuner_name, bump):
            b.add(1023, 12345, full_cigar(cs, 1023, widest=True), name_len=254, mds=md)
        b.specs[LONG_B] = dict(b.specs[LONG_B], rlen=b_read, pos=777, els=full_cigar(cs, b_read, widest=True), name_len=b_name, mds=list(md or []),
                               mds_len=None, state=ALIGNED)
        return b.build(cs, ms)

    # LONG_B: reads first (1.5 or 2 bytes a base), then the name (1 byte a byte), until it has cap - 3 bytes
    b_name, b_read = 8, shape["mrl"] + 1
    for _ in range(16):
        have = record_bytes(fmt, refs, build(1, {}, b_name, b_read), LONG_B)
        if have == cap - 3:
            break
        if (cap - 3 - have) // 2 - 1 >= 1 and b_read < 1020:
            b_read = min(1020, b_read + (cap - 3 - have) // 2 - 1)
        else:
            b_name += cap - 3 - have
    assert have == cap - 3 and 1 <= b_name <= 254 and b_read > shape["mrl"], (have, cap, b_name, b_read)
    sized = lambda t, bump: build(t, bump, b_name, b_read)
    return refs, sized(*_spread(fmt, refs, sized, 37, LONG_B, 9)), shape, cap


# ---- MDS streams that end inside a token -------------------------------------------------------------------------------------------
CUT_STRIDES = (4, 16, 64)


def _cut_streams(stride):
    """[(what, the stride's bytes of a stream cut there)]: mismatch tokens fill the stream up to the token that is cut after `keep` bytes"""
    out = []
    for what, token, keeps in (("deletion of 255", [3, 255] + [k % 4 for k in range(255)], (1, 2, 6)), ("match run", [0, 77], (1, 2)),
                               ("mismatch", [1, 3], (1, 2)), ("insertion", [2, 5, 1, 2, 3, 0, 1], (1, 2, 4))):
        for keep in keeps:
            fill = stride - 2 - keep
            if fill < 0:
                continue
            tokens = ([[3, 1, 2]] if fill % 2 else []) + [[1, (k + 1) % 4] for k in range((fill - 3 * (fill % 2)) // 2)]
            if fill == 1:
                continue
            full = mds_stream(tokens + [token, [0, 9]])
            out.append(("%s cut after %d" % (what, keep), full[:stride], len(full)))
    return out


@functools.lru_cache(None)
def cut_md_batch(fmt, stride):
    """every cut stream four times: a short read and a read of max_read_len, each with mds_lens equal to the stride and with the whole
    stream's length (above it); then the same stream ending one byte BEFORE the stride with 0xFF behind it in the row, which must read
    as 0.  max_read_len is the longest that keeps (20, 5, 4, max_read_len, stride) in the smallest class, so that a long read with a cut
    deletion of 255 does not fit and a short one does.  -> (refs, rec, shape, cap)"""
    smallest = (SAM_CLASSES if fmt == "sam" else BAM_CLASSES)[0]
    mrl = max(m for m in range(1, 1024) if need_of(fmt, dict(name=20, ref_name=5, cs=4, mrl=m, ms=stride)) <= smallest)
    shape = _shape(fmt, 20, 5, 4, mrl, stride, "cut MD, stride %d" % stride)
    refs = class_refs(5)
    b = Batch()
    for what, row, full_len in _cut_streams(stride):
        for rlen in (10, mrl):
            for mds_len in (stride, full_len):
                if rlen == mrl:                                                         # the most text around the MD: 5-digit deletions, a 9-digit POS
                    b.add(rlen, (1 << 29) - 120000 + 1000 * len(b.specs), full_cigar(4, rlen, widest=True), name_len=20, mds=row, mds_len=mds_len)
                else:
                    b.add(rlen, 4000 + 1000 * len(b.specs), [(rlen, M_)], mds=row, mds_len=mds_len)
        b.add(10, 4000, [(10, M_)], mds=row[:stride - 1] + [255], mds_len=stride - 1)
    return refs, b.build(4, stride), shape, smallest - _stage(stride)


# ---- BGZF --------------------------------------------------------------------------------------------------------------------------
# the payloads the framing kernel is run on: eight blocks with a one-byte last block, eight whole blocks, nine blocks whose last has a row
# (4096 bytes) and a byte, and seventeen blocks.  A framed block has 65280 + 31 bytes and its payload starts 23 bytes in, so block b cuts its 16-byte words
# at the byte shift bgzf_shift(b): 9, 10, ..., 15, 0, 1, ..., 8 over sixteen blocks -- every value once
BGZF_SIZES = (7 * 65280 + 1, 8 * 65280, 8 * 65280 + 4097, 16 * 65280 + 4097)


def bgzf_shift(b):
    return (16 - (b * (65280 + 31) + 23) % 16) % 16


# ---- the scan's carry --------------------------------------------------------------------------------------------------------------
SCAN_N = 1024 * 2048 + 2048 + 5                                       # n + 1 values: 1026 tiles of 2048, two of them in the second round


@functools.lru_cache(None)
def scan_batch_41():
    """41 unaligned records: names of 1 ... 3 bytes, reads of 1 ... 4 bases"""
    b = Batch()
    for j in range(41):
        b.add(1 + (j * 3) % 4, name_len=1 + (j * 2) % 3)
    return many_refs(3), b.build(1, None)
