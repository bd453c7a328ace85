"""A plain-Python restatement of the SAM record format (include/nvbio_amd.h, "SAM output"), written from the rules
-- the behaviour of the reference's io::SamOutput -- and not from the kernels.  The tests compare the library's bytes with it.

refs    : dict(sequence_index = uint32 [n_seqs + 1], names = [bytes] * n_seqs)
records : dict(names = [bytes] * n, reads = uint8 [sum of lengths] (the STORED symbols, 0..15), read_index = uint32 [n + 1],
               quals = uint8 [sum of lengths] or None, state = uint8 [n] (bit 0 aligned, 1 rc, 2 read 2, 3 paired), pos = uint32 [n],
               score = int32 [n], second_score = int32 [n] or None, ed = uint32 [n], mapq = uint8 [n], cigars = uint16 [n, cigar_stride]
               (backtracking order, len << 2 | op), cigar_lens = uint32 [n], mds = uint8 [n, mds_stride] or None, mds_lens = uint32 [n],
               mate_of = uint32 [n] or None, reads_reversed = True)
"""
import numpy as np

SCORE_MIN = -(1 << 30)
U32 = 0xFFFFFFFF


def dna_char(s):
    return "ACGT"[s] if s < 4 else "N"


def pack4(symbols):
    """4-bit big-endian packing into uint32 words: symbol i in bits [28 - 4 (i & 7), 31 - 4 (i & 7)] of word i >> 3"""
    s = np.asarray(symbols, dtype=np.uint32)
    pad = (-len(s)) % 8
    s = np.concatenate([s, np.zeros(pad, np.uint32)]).reshape(-1, 8)
    w = np.zeros(len(s), dtype=np.uint32)
    for k in range(8):
        w |= s[:, k] << np.uint32(28 - 4 * k)
    return w if len(w) else np.zeros(1, np.uint32)


def cigar_elements(rec, i):
    """the elements of record i, or None when the CIGAR was truncated"""
    n = int(rec["cigar_lens"][i])
    if n > rec["cigars"].shape[1]:
        return None
    return [(int(c) >> 2, int(c) & 3) for c in rec["cigars"][i, :n]]


def reference_length(els):
    return sum(l for l, t in els if t in (0, 2))


def md_and_counts(rec, i):
    """generate_md_string -> (MD text, XM, XO, XG); the merged match run is summed without wrapping"""
    if rec.get("mds") is None:
        return "", 0, 0, 0
    n = min(int(rec["mds_lens"][i]), rec["mds"].shape[1])
    if n <= 2:
        return "", 0, 0, 0
    m = rec["mds"][i]
    B = lambda k: int(m[k]) if k < n else 0
    out, mm, gapo, gape = [], 0, 0, 0
    k = 2
    while True:
        op = B(k)
        k += 1
        if op == 0:
            l = B(k)
            k += 1
            while k < n and m[k] == 0:
                l += B(k + 1)
                k += 2
            out.append(str(l))
        elif op == 1:
            out.append(dna_char(B(k)))
            k += 1
            mm += 1
        elif op == 2:
            l = B(k)
            k += 1 + l
            gapo += 1
            gape += l - 1
        elif op == 3:
            l = B(k)
            k += 1
            out.append("^" + "".join(dna_char(B(k + j)) for j in range(l)) + "0")
            k += l
            gapo += 1
            gape += l - 1
        if k >= n:
            break
    return "".join(out), mm, gapo, gape


def seq_and_qual(rec, i):
    b, e = int(rec["read_index"][i]), int(rec["read_index"][i + 1])
    rc = (int(rec["state"][i]) >> 1) & 1
    stored = [int(x) for x in rec["reads"][b:e]]
    quals = None if rec.get("quals") is None else [int(x) for x in rec["quals"][b:e]]
    flip = (not rc) if rec.get("reads_reversed", True) else bool(rc)
    if flip:
        stored = stored[::-1]
        quals = None if quals is None else quals[::-1]
    if rc:
        stored = [3 - s if s < 4 else 4 for s in stored]
    seq = "".join(dna_char(s) for s in stored)
    qual = "*" if quals is None else "".join(chr((q + 33) & 0xFF) for q in quals)
    return seq, qual


def sequence_of(refs, pos):
    si = refs["sequence_index"]
    return max(int(np.searchsorted(si[:len(refs["names"])], pos, side="right")) - 1, 0)


def sam_record(refs, rec, i):
    """the bytes of record i, or None for a record that is skipped"""
    st = int(rec["state"][i])
    name = rec["names"][i].decode("latin-1")
    seq, qual = seq_and_qual(rec, i)
    short = lambda flags: ("%s\t%d\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (name, flags, seq, qual)).encode("latin-1")
    if not st & 1:
        return short(4)
    els = cigar_elements(rec, i)
    rlen = int(rec["read_index"][i + 1]) - int(rec["read_index"][i])
    if els is None or sum(l for l, t in els if t != 2) != rlen:
        return None
    si = refs["sequence_index"]
    pos = int(rec["pos"][i])
    s = sequence_of(refs, pos)
    flags = (128 if st & 4 else 64) | (16 if st & 2 else 0)
    mate = None if rec.get("mate_of") is None else int(rec["mate_of"][i])
    if mate is not None:
        ms = int(rec["state"][mate])
        flags |= 1 | (2 if ms & 8 else 0) | (0 if ms & 1 else 8) | (32 if ms & 2 else 0)
    ref_len = reference_length(els)
    if ((pos + ref_len) & U32) > int(si[s + 1]):
        return short(flags | 4)
    own = (pos - int(si[s]) + 1) & U32
    cigar = "".join("%d%s" % (l, "MIDS"[t]) for l, t in reversed(els))
    if mate is None:
        nxt = "*\t0\t0"
    elif int(rec["state"][mate]) & 1:
        mpos = int(rec["pos"][mate])
        ms_ = sequence_of(refs, mpos)
        mref = reference_length(cigar_elements(rec, mate) or [])
        tlen = 0
        if ms_ == s:
            tlen = (max((mpos + mref) & U32, (pos + ref_len) & U32) - min(mpos, pos)) & U32
            tlen = tlen - (1 << 32) if tlen >= 1 << 31 else tlen
            if mpos < pos:
                tlen = -tlen
        nxt = "%s\t%d\t%d" % ("=" if ms_ == s else refs["names"][ms_].decode("latin-1"), (mpos - int(si[ms_]) + 1) & U32, tlen)
    else:
        nxt = "=\t%d\t0" % own
    md, mm, gapo, gape = md_and_counts(rec, i)
    tags = "NM:i:%d\tAS:i:%d" % (int(rec["ed"][i]) & U32, int(rec["score"][i]))
    if rec.get("second_score") is not None and int(rec["second_score"][i]) != SCORE_MIN:
        tags += "\tXS:i:%d" % int(rec["second_score"][i])
    tags += "\tXM:i:%d\tXO:i:%d\tXG:i:%d\tMD:Z:%s" % (mm, gapo, gape, md or "*")
    return ("%s\t%d\t%s\t%d\t%d\t%s\t%s\t%s\t%s\t%s\n" % (name, flags, refs["names"][s].decode("latin-1"), own, int(rec["mapq"][i]), cigar, nxt, seq,
                                                         qual, tags)).encode("latin-1")


def sam_records(refs, rec):
    """-> (text bytes, offsets int64 [n + 1], n_skipped)"""
    n = len(rec["names"])
    parts = [sam_record(refs, rec, i) for i in range(n)]
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([0 if p is None else len(p) for p in parts]) if n else 0
    return b"".join(p for p in parts if p is not None), offsets, sum(p is None for p in parts)


def sam_header(names, lengths, pg_id="nvBowtie", pg_name="nvBowtie", pg_version="0.5.1"):
    lines = ["@HD\tVN:1.3", "@PG\tID:%s\tPN:%s\tVN:%s" % (pg_id, pg_name, pg_version)]
    lines += ["@SQ\tSN:%s\tLN:%d" % (n.decode("latin-1") if isinstance(n, bytes) else n, l) for n, l in zip(names, lengths)]
    return ("\n".join(lines) + "\n").encode("latin-1")


# ---- random inputs for the GPU tests ---------------------------------------------------------------------------------------------------
SPECIAL_LENS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023)
M_, I_, D_, S_ = 0, 1, 2, 3


def random_refs():
    """three sequences with names of different lengths"""
    return dict(sequence_index=np.array([0, 50000, 120000, 150000], np.uint32), names=[b"chr1", b"chrUn_gl000220.1", b"MT"])


def _digits_len(rng):
    """a length of 1 to 4 digits, each width as likely"""
    lo, hi = ((1, 10), (10, 100), (100, 1000), (1000, 3000))[int(rng.integers(0, 4))]
    return int(rng.integers(lo, hi))


def _random_cigar(rng, read_len, stride, full):
    """elements (backtracking order is just an order: any list will do) whose non-D lengths sum to read_len, `full`: exactly `stride` of them"""
    k = stride if full else int(rng.integers(1, stride + 1))
    m = int(min(read_len, rng.integers(1, k + 1)))                    # the elements that consume the read
    cuts = np.sort(rng.choice(np.arange(1, read_len), m - 1, replace=False)) if m > 1 else np.array([], np.int64)
    parts = np.diff(np.concatenate([[0], cuts, [read_len]]))
    els = [(int(p), int(rng.choice([M_, M_, I_, S_]))) for p in parts] + [(_digits_len(rng), D_) for _ in range(k - m)]
    order = rng.permutation(len(els))
    return [els[j] for j in order]


def _random_mds(rng, kind):
    """an MDS stream: kind 0 empty (length 0), 1 two bytes, 2 a deletion of 255 between adjacent tokens, 3 longer than any stride here, else random"""
    if kind == 0:
        return []
    tokens = []
    if kind == 2:
        tokens = [[0, 255], [0, 255], [0, 7], [1, 2], [1, 4], [3, 255] + [int(x) for x in rng.integers(0, 5, 255)], [3, 1, 3], [2, 2, 0, 1], [0, 1]]
    elif kind == 3:
        tokens = [[3, 255] + [int(x) for x in rng.integers(0, 5, 255)] for _ in range(2)] + [[0, 9]]
    elif kind != 1:
        for _ in range(int(rng.integers(1, 14))):
            t = int(rng.integers(0, 4))
            if t == 0:
                tokens.append([0, int(rng.integers(1, 256))])
            elif t == 1:
                tokens.append([1, int(rng.integers(0, 5))])
            else:
                l = int(rng.integers(1, 6))
                tokens.append([t, l] + [int(x) for x in rng.integers(0, 5, l)])
    body = [b for t in tokens for b in t]
    n = len(body) + 2
    return [n & 255, n >> 8] + body


def random_records(rng, n, refs, quals=True, paired=False, cigar_stride=8, mds_stride=320, special_lens=SPECIAL_LENS):
    """n records over `refs` with every feature the format has (see tests/test_gpu_sam.py for what is asserted about them); paired:
    records 2p and 2p + 1 are each other's mates (n even), anchor first"""
    si = refs["sequence_index"].astype(np.int64)
    lens = [int(rng.integers(1, 301)) for _ in range(n)]
    for j, l in enumerate(special_lens[:n]):
        lens[(j * 21 + 3) % n if n > len(special_lens) else j] = l
    if paired:
        lens = [int(rng.integers(30, 120)) for _ in range(n)]
    names = [bytes(rng.integers(33, 127, int(rng.integers(1, 41))).astype(np.uint8)) for _ in range(n)]
    read_index = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total = int(read_index[-1])
    reads = rng.integers(0, 4, total).astype(np.uint8)
    reads[rng.random(total) < 0.03] = 4
    reads[rng.random(total) < 0.005] = 15                              # every other 4-bit code prints N too
    state = np.zeros(n, np.uint8)
    pos = np.zeros(n, np.uint32)
    cigars = np.zeros((n, cigar_stride), np.uint16)
    cigar_lens = np.zeros(n, np.uint32)
    mds = np.zeros((n, mds_stride), np.uint8)
    mds_lens = np.zeros(n, np.uint32)
    for i in range(n):
        aligned = rng.random() < 0.8
        read_2 = ((i & 1) ^ int((i >> 1) % 3 == 0)) if paired else int(rng.random() < 0.5)      # the anchor of every third pair is read 2
        state[i] = (1 if aligned else 0) | (2 if rng.random() < 0.5 else 0) | (4 if read_2 else 0) | (8 if rng.random() < 0.5 else 0)
        els = _random_cigar(rng, lens[i], cigar_stride, full=(i % 7 == 0) and lens[i] >= 1)
        cigar_lens[i] = len(els)
        how = rng.random()
        if aligned and not paired and how < 0.02:
            cigar_lens[i] = cigar_stride + 1                            # truncated
        elif aligned and not paired and how < 0.04:
            cigar_lens[i] = 0xFFFFFFFF
        elif aligned and not paired and how < 0.07:
            j = next(k for k, e in enumerate(els) if e[1] != D_)
            els[j] = (els[j][0] + 1, els[j][1])                         # the lengths no longer sum to the read's
        cigars[i, :len(els)] = [l << 2 | t for l, t in els]
        ref_len = sum(l for l, t in els if t in (M_, D_))
        s = int(rng.integers(0, len(refs["names"])))
        if paired and i & 1 and rng.random() < 0.7:
            s = int(np.searchsorted(si, int(pos[i - 1]), side="right")) - 1     # the anchor's sequence
        where = rng.random()
        room = int(si[s + 1] - si[s])
        if where < 0.08:
            p = si[s + 1] - ref_len + int(rng.integers(1, 6))           # ends past its sequence (or, on the last one, past the genome)
        elif where < 0.14:
            p = si[s + 1] - ref_len                                     # ends exactly with it
        elif paired and i & 1 and where < 0.8:
            p = int(pos[i - 1]) + int(rng.integers(-400, 400))          # near the anchor, before or behind
        else:
            p = si[s] + int(rng.integers(0, max(room - ref_len, 1)))
        pos[i] = int(min(max(p, si[s]), si[s + 1] - 1))
        kind = i % 16 if i % 16 < 4 else 9
        m = _random_mds(rng, kind)
        mds_lens[i] = len(m)
        mds[i, :min(len(m), mds_stride)] = m[:mds_stride]
    rec = dict(names=names, reads=reads, read_index=read_index, quals=rng.integers(0, 94, total).astype(np.uint8) if quals else None, state=state, pos=pos,
               score=rng.integers(-65536, 2047, n).astype(np.int32),
               second_score=np.where(rng.random(n) < 0.5, SCORE_MIN, rng.integers(-65536, 2047, n)).astype(np.int32),
               ed=rng.integers(0, 301, n).astype(np.uint32), mapq=rng.integers(0, 256, n).astype(np.uint8), cigars=cigars, cigar_lens=cigar_lens, mds=mds,
               mds_lens=mds_lens, mate_of=(np.arange(n, dtype=np.uint32) ^ 1) if paired else None, reads_reversed=True)
    if n:
        rec["score"][0], rec["score"][n - 1] = -65536, 2046
    return rec
