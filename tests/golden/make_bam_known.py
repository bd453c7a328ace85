"""Writes tests/golden/bam_known.bin: seven BAM records worked out BY HAND, byte by byte, from the rules of the record format
(include/nvbio_amd.h "BAM output") over the inputs of tests/golden/sam_known.npz (make_sam_known.py holds them; this
file reads nothing and changes nothing there).  Nothing here calls the restatement (tests/bam_cpu.py) or the library: the test pins
the restatement's encoder against these bytes.

Every integer is little-endian.  A record: block_size (the bytes after it) | refID | pos | bin_mq_nl = bin << 16 | mapq << 8 | l_read_name
| flag_nc = flag << 16 | n_cigar_op | l_seq | next_refID | next_pos | tlen | QNAME NUL | CIGAR (len << 4 | op, M I D S = 0 1 2 4) | SEQ
(A C G T N = 1 2 4 8 15, high nibble first) | QUAL (raw) | tags.  chr1 = [0, 1000) is refID 0, chrB = [1000, 1500) refID 1."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# (which records of sam_known.npz: "se" / "pe", index), in the order of the file
ORDER = [("se", 0), ("se", 2), ("se", 3), ("se", 6), ("pe", 2), ("pe", 3), ("pe", 4)]

ACGTACGT = "12 48 12 48"                      # what every FWD8 read prints, 8 symbols in 4 bytes
Q40x8 = "28 28 28 28 28 28 28 28"
TAGS8 = """
    4e 4d 63 00                               # NM c 0
    41 53 69 00 00 00 00                      # AS i 0            (no XS: the second score is SCORE_MIN)
    58 4d 63 00  58 4f 63 00  58 47 63 00     # XM XO XG c 0
    4d 44 5a 38 00                            # MD Z "8" NUL
"""

RECORDS = [
    # r0: not aligned, stored ACGTN (reversed storage, so it prints NTGCA), qualities 0..4 turned round with it
    """
    2b 00 00 00                               # block_size 43 = 32 + 3 + 3 + 5
    ff ff ff ff  ff ff ff ff                  # refID -1, pos -1
    03 00 00 00                               # bin_mq_nl: l_read_name 3 alone, no MAPQ
    00 00 04 00                               # flag_nc: 4 << 16 exactly, no CIGAR
    05 00 00 00                               # l_seq 5
    ff ff ff ff  ff ff ff ff  00 00 00 00     # next_refID -1, next_pos -1, tlen 0
    72 30 00                                  # "r0" NUL
    f8 42 10                                  # N T | G C | A 0
    04 03 02 01 00                            # QUAL
    """,
    # rcN: rc on chrB at 1004 (pos 4), stored ACNGT -> complemented in stored order TGNCA, XS present, MD 2N2
    """
    55 00 00 00                               # block_size 85 = 32 + 4 + 4 + 3 + 5 + 4 + 7 + 7 + 12 + 7
    01 00 00 00  04 00 00 00                  # refID 1, pos 4
    04 03 00 00                               # l_read_name 4 | mapq 3 << 8, bin 0
    01 00 50 00                               # flag 80 = 64 | 16, one CIGAR element
    05 00 00 00                               # l_seq 5
    ff ff ff ff  ff ff ff ff  00 00 00 00     # single-end: -1, -1, 0
    72 63 4e 00                               # "rcN" NUL
    50 00 00 00                               # 5M
    84 f2 10                                  # T G | N C | A 0
    0a 14 1e 28 29                            # QUAL in stored order
    4e 4d 63 01                               # NM c 1
    41 53 69 ff ff ff ff                      # AS i -1
    58 53 69 f9 ff ff ff                      # XS i -7
    58 4d 63 01  58 4f 63 00  58 47 63 00     # XM 1, XO 0, XG 0
    4d 44 5a 32 4e 32 00                      # MD Z "2N2" NUL
    """,
    # del: 150 x C on chr1 at 200, CIGAR kept as 3M 2D 147M (backtracking order) -> 147M 2D 3M, MD 147^AT03, MAPQ 255
    """
    34 01 00 00                               # block_size 308 = 32 + 4 + 12 + 75 + 150 + 4 + 7 + 12 + 12
    00 00 00 00  c8 00 00 00                  # refID 0, pos 200
    04 ff 00 00                               # l_read_name 4 | mapq 255 << 8
    03 00 40 00                               # flag 64, three CIGAR elements
    96 00 00 00                               # l_seq 150
    ff ff ff ff  ff ff ff ff  00 00 00 00
    64 65 6c 00                               # "del" NUL
    30 09 00 00  22 00 00 00  30 00 00 00     # 147M (147 << 4 = 0x930), 2D (2 << 4 | 2), 3M
    """ + "22 " * 75 + """                    # SEQ: C C, 75 times
    """ + "1e " * 150 + """                   # QUAL 30, 150 times
    4e 4d 63 02                               # NM c 2
    41 53 69 f5 ff ff ff                      # AS i -11
    58 4d 63 00  58 4f 63 01  58 47 63 01     # XM 0, XO 1, XG 1 (one gap of two)
    4d 44 5a 31 34 37 5e 41 54 30 33 00       # MD Z "147^AT03" NUL
    """,
    # straddle: 8M at 996 ends at 1004, past chr1's 1000: 4 ORed into 64, every reference field -1, no CIGAR, no MAPQ, no tags
    """
    35 00 00 00                               # block_size 53 = 32 + 9 + 4 + 8
    ff ff ff ff  ff ff ff ff                  # refID -1, pos -1
    09 00 00 00                               # l_read_name 9 alone (MAPQ 42 is not written)
    00 00 44 00                               # flag 68, n_cigar_op 0
    08 00 00 00                               # l_seq 8
    ff ff ff ff  ff ff ff ff  00 00 00 00
    73 74 72 61 64 64 6c 65 00                # "straddle" NUL
    """ + ACGTACGT + """
    """ + Q40x8 + """
    """,
    # pB/1: chr1 at 50, its mate pB/2 on chrB at 1200: next_refID is the MATE'S SEQUENCE (1), next_pos 200 within it, tlen 0 across sequences
    """
    51 00 00 00                               # block_size 81 = 32 + 5 + 4 + 4 + 8 + 4 + 7 + 12 + 5
    00 00 00 00  32 00 00 00                  # refID 0, pos 50
    05 1e 00 00                               # l_read_name 5 | mapq 30 << 8
    01 00 41 00                               # flag 65 = 64 | 1 (the mate is not paired, is aligned, is not rc)
    08 00 00 00
    01 00 00 00  c8 00 00 00  00 00 00 00     # next_refID 1, next_pos 200, tlen 0
    70 42 2f 31 00                            # "pB/1" NUL
    80 00 00 00                               # 8M
    """ + ACGTACGT + """
    """ + Q40x8 + TAGS8,
    # pB/2: the other way round: refID 1, next_refID 0 (the reference would write the difference, -1: divergence 2)
    """
    51 00 00 00
    01 00 00 00  c8 00 00 00                  # refID 1, pos 200
    05 1e 00 00
    01 00 81 00                               # flag 129 = 128 | 1
    08 00 00 00
    00 00 00 00  32 00 00 00  00 00 00 00     # next_refID 0, next_pos 50, tlen 0
    70 42 2f 32 00                            # "pB/2" NUL
    80 00 00 00
    """ + ACGTACGT + """
    """ + Q40x8 + TAGS8,
    # pC/1: rc on chr1 at 700, its mate not aligned: flag 89 = 64 | 16 | 1 | 8, next_refID = refID, next_pos = pos, tlen 0
    """
    51 00 00 00
    00 00 00 00  bc 02 00 00                  # refID 0, pos 700
    05 1e 00 00
    01 00 59 00                               # flag 89
    08 00 00 00
    00 00 00 00  bc 02 00 00  00 00 00 00     # next_refID 0, next_pos 700, tlen 0
    70 43 2f 31 00                            # "pC/1" NUL
    80 00 00 00
    """ + ACGTACGT + """                      # stored TGCATGCA complemented in stored order
    """ + Q40x8 + TAGS8,
]


def record_bytes(text):
    return bytes.fromhex("".join(line.split("#")[0] for line in text.splitlines()))


if __name__ == "__main__":
    data = b"".join(record_bytes(r) for r in RECORDS)
    with open(os.path.join(HERE, "bam_known.bin"), "wb") as f:
        f.write(data)
    print("%d records, %d bytes" % (len(RECORDS), len(data)))
