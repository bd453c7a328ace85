"""Writes tests/golden/sam_known.npz and sam_known.txt: 24 SAM records worked out BY HAND from the rules of the record format
(include/nvbio_amd.h "SAM output") -- the input arrays here, the expected lines spelled out below.  Nothing in this
file calls the restatement (tests/sam_cpu.py) or the library: the test pins both against these lines.

Reference: chr1 = [0, 1000), chrB = [1000, 1500).  Reads are stored reversed (nvBowtie); symbols A C G T N = 0 1 2 3 4.
A CIGAR element is len << 2 | op with ops M I D S = 0 1 2 3, kept in backtracking order (last element first).
An MDS stream is 2 length bytes (its own length, low byte first), then [0, run] / [1, symbol] / [2, n, symbols...] (insertion) /
[3, n, symbols...] (deletion)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SCORE_MIN = -(1 << 30)
SYM = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
M, I, D, S = 0, 1, 2, 3
CIGAR_STRIDE, MDS_STRIDE = 4, 16


def el(length, op):
    return length << 2 | op


def mds(*tokens):
    body = [b for t in tokens for b in t]
    n = len(body) + 2
    return [n & 255, n >> 8] + body


MD8 = mds([0, 8])                                   # eight matches
FWD8 = dict(stored="TGCATGCA", quals=[40] * 8)      # the read ACGTACGT stored reversed; as an rc alignment's stored read it prints ACGTACGT too


def rec(name, state, stored, quals, pos=0, score=0, second=SCORE_MIN, ed=0, mapq=0, cigar=(), cigar_len=None, md=()):
    return dict(name=name, state=state, stored=stored, quals=quals, pos=pos, score=score, second=second, ed=ed, mapq=mapq, cigar=list(cigar),
                cigar_len=len(cigar) if cigar_len is None else cigar_len, md=list(md))


# ---- single-end: state bit 0 aligned, bit 1 rc, bit 2 read 2 -----------------------------------------------------------------------
SE = [
    rec("r0", 0, "ACGTN", [0, 1, 2, 3, 4]),
    rec("read/1", 1, pos=99, mapq=42, cigar=[el(8, M)], md=MD8, **FWD8),
    rec("rcN", 3, "ACNGT", [10, 20, 30, 40, 41], pos=1004, score=-1, second=-7, ed=1, mapq=3, cigar=[el(5, M)], md=mds([0, 2], [1, 4], [0, 2])),
    rec("del", 1, "C" * 150, [30] * 150, pos=200, score=-11, ed=2, mapq=255, cigar=[el(3, M), el(2, D), el(147, M)],
        md=mds([0, 147], [3, 2, 0, 3], [0, 3])),
    rec("clip", 1, "TTCATGCAGG", [0] * 10, pos=9, score=12, second=5, cigar=[el(2, S), el(6, M), el(2, S)], md=mds([2, 2, 2, 2], [0, 6], [2, 2, 3, 3])),
    rec("run300", 1 | 4, "A" * 300, [40] * 300, pos=500, mapq=40, cigar=[el(300, M)], md=mds([0, 255], [0, 45])),
    rec("straddle", 1, pos=996, mapq=42, cigar=[el(8, M)], md=MD8, **FWD8),
    rec("edge", 1, pos=992, mapq=1, cigar=[el(8, M)], md=MD8, **FWD8),
    rec("trunc", 1, pos=10, cigar=[el(2, M)] * 4, cigar_len=5, md=MD8, **FWD8),
    rec("trunc2", 1, pos=10, cigar=[el(8, M)], cigar_len=0xFFFFFFFF, md=MD8, **FWD8),
    rec("badsum", 1, pos=10, cigar=[el(7, M)], md=MD8, **FWD8),
    rec("ins", 3, "TGCATGCA", [1, 2, 3, 4, 5, 6, 7, 8], pos=1100, score=-20, second=-20, ed=3, mapq=7, cigar=[el(4, M), el(1, I), el(3, M)],
        md=mds([0, 1], [1, 0], [1, 1], [2, 1, 3], [0, 4])),
    rec("nomd", 1, pos=0, mapq=9, cigar=[el(8, M)], md=[], **FWD8),
    rec("unrc", 2, "AACC", [5, 6, 7, 8]),
]
SE_LINES = [
    "r0\t4\t*\t0\t0\t*\t*\t0\t0\tNTGCA\t%$#\"!",
    "read/1\t64\tchr1\t100\t42\t8M\t*\t0\t0\tACGTACGT\tIIIIIIII\tNM:i:0\tAS:i:0\tXM:i:0\tXO:i:0\tXG:i:0\tMD:Z:8",
    "rcN\t80\tchrB\t5\t3\t5M\t*\t0\t0\tTGNCA\t+5?IJ\tNM:i:1\tAS:i:-1\tXS:i:-7\tXM:i:1\tXO:i:0\tXG:i:0\tMD:Z:2N2",
    "del\t64\tchr1\t201\t255\t147M2D3M\t*\t0\t0\t" + "C" * 150 + "\t" + "?" * 150 + "\tNM:i:2\tAS:i:-11\tXM:i:0\tXO:i:1\tXG:i:1\tMD:Z:147^AT03",
    "clip\t64\tchr1\t10\t0\t2S6M2S\t*\t0\t0\tGGACGTACTT\t!!!!!!!!!!\tNM:i:0\tAS:i:12\tXS:i:5\tXM:i:0\tXO:i:2\tXG:i:2\tMD:Z:6",
    "run300\t128\tchr1\t501\t40\t300M\t*\t0\t0\t" + "A" * 300 + "\t" + "I" * 300 + "\tNM:i:0\tAS:i:0\tXM:i:0\tXO:i:0\tXG:i:0\tMD:Z:300",
    "straddle\t68\t*\t0\t0\t*\t*\t0\t0\tACGTACGT\tIIIIIIII",
    "edge\t64\tchr1\t993\t1\t8M\t*\t0\t0\tACGTACGT\tIIIIIIII\tNM:i:0\tAS:i:0\tXM:i:0\tXO:i:0\tXG:i:0\tMD:Z:8",
    None,                                             # trunc: cigar_len 5 > cigar_stride 4
    None,                                             # trunc2: cigar_len 0xFFFFFFFF
    None,                                             # badsum: 7M for a read of 8
    "ins\t80\tchrB\t101\t7\t3M1I4M\t*\t0\t0\tACGTACGT\t\"#$%&'()\tNM:i:3\tAS:i:-20\tXS:i:-20\tXM:i:2\tXO:i:1\tXG:i:0\tMD:Z:1AC4",
    "nomd\t64\tchr1\t1\t9\t8M\t*\t0\t0\tACGTACGT\tIIIIIIII\tNM:i:0\tAS:i:0\tXM:i:0\tXO:i:0\tXG:i:0\tMD:Z:*",
    "unrc\t4\t*\t0\t0\t*\t*\t0\t0\tTTGG\t&'()",
]

# ---- paired: bit 3 = paired; record i's mate is PE_MATE[i] ------------------------------------------------------------------------------
TAGS8 = "\tNM:i:0\tAS:i:0\tXM:i:0\tXO:i:0\tXG:i:0\tMD:Z:8"
pe = lambda name, state, pos=0: rec(name, state, pos=pos, mapq=30, cigar=[el(8, M)], md=MD8, **FWD8)
PE = [
    pe("pA/1", 1 | 8, 100), pe("pA/2", 1 | 2 | 4 | 8, 300),       # the same sequence, the mate behind / before, the mate rc, both paired
    pe("pB/1", 1, 50), pe("pB/2", 1 | 4, 1200),                   # different sequences, not paired
    pe("pC/1", 1 | 2, 700), pe("pC/2", 4),                        # the mate unaligned
    pe("pD/1", 0), pe("pD/2", 4),                                 # both unaligned
    pe("pE/1", 1 | 8, 996), pe("pE/2", 1 | 2 | 4 | 8, 900),       # a straddler and its mate
]
PE_MATE = [1, 0, 3, 2, 5, 4, 7, 6, 9, 8]
PE_LINES = [
    "pA/1\t99\tchr1\t101\t30\t8M\t=\t301\t208\tACGTACGT\tIIIIIIII" + TAGS8,
    "pA/2\t147\tchr1\t301\t30\t8M\t=\t101\t-208\tACGTACGT\tIIIIIIII" + TAGS8,
    "pB/1\t65\tchr1\t51\t30\t8M\tchrB\t201\t0\tACGTACGT\tIIIIIIII" + TAGS8,
    "pB/2\t129\tchrB\t201\t30\t8M\tchr1\t51\t0\tACGTACGT\tIIIIIIII" + TAGS8,
    "pC/1\t89\tchr1\t701\t30\t8M\t=\t701\t0\tACGTACGT\tIIIIIIII" + TAGS8,
    "pC/2\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGT\tIIIIIIII",
    "pD/1\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGT\tIIIIIIII",
    "pD/2\t4\t*\t0\t0\t*\t*\t0\t0\tACGTACGT\tIIIIIIII",
    "pE/1\t103\t*\t0\t0\t*\t*\t0\t0\tACGTACGT\tIIIIIIII",
    "pE/2\t147\tchr1\t901\t30\t8M\t=\t997\t104\tACGTACGT\tIIIIIIII" + TAGS8,
]
HEADER = ["@HD\tVN:1.3", "@PG\tID:nvBowtie\tPN:nvBowtie\tVN:0.5.1", "@SQ\tSN:chr1\tLN:1000", "@SQ\tSN:chrB\tLN:500"]


def arrays(prefix, records, mate_of=None):
    n = len(records)
    names = [r["name"].encode() for r in records]
    out = {"names": np.frombuffer(b"".join(names), np.uint8), "name_index": np.cumsum([0] + [len(x) for x in names]).astype(np.uint32),
           "reads": np.array([SYM[c] for r in records for c in r["stored"]], np.uint8),
           "read_index": np.cumsum([0] + [len(r["stored"]) for r in records]).astype(np.uint32),
           "quals": np.array([q for r in records for q in r["quals"]], np.uint8)}
    for key, field, dtype in (("state", "state", np.uint8), ("pos", "pos", np.uint32), ("score", "score", np.int32), ("second_score", "second", np.int32),
                              ("ed", "ed", np.uint32), ("mapq", "mapq", np.uint8), ("cigar_lens", "cigar_len", np.uint32)):
        out[key] = np.array([r[field] for r in records], dtype)
    out["cigars"] = np.zeros((n, CIGAR_STRIDE), np.uint16)
    out["mds"] = np.zeros((n, MDS_STRIDE), np.uint8)
    out["mds_lens"] = np.array([len(r["md"]) for r in records], np.uint32)
    for i, r in enumerate(records):
        out["cigars"][i, :len(r["cigar"])] = r["cigar"]
        out["mds"][i, :len(r["md"])] = r["md"]
    if mate_of is not None:
        out["mate_of"] = np.array(mate_of, np.uint32)
    return {prefix + k: v for k, v in out.items()}


if __name__ == "__main__":
    ref_names = [b"chr1", b"chrB"]
    z = dict(sequence_index=np.array([0, 1000, 1500], np.uint32), ref_names=np.frombuffer(b"".join(ref_names), np.uint8),
             ref_names_index=np.array([0, 4, 8], np.uint32))
    z.update(arrays("se_", SE))
    z.update(arrays("pe_", PE, PE_MATE))
    np.savez_compressed(os.path.join(HERE, "sam_known.npz"), **z)
    lines = HEADER + [x for x in SE_LINES + PE_LINES if x is not None]
    with open(os.path.join(HERE, "sam_known.txt"), "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("latin-1"))
    print("%d records, %d lines" % (len(SE) + len(PE), len(lines)))
