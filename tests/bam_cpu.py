"""A plain-Python restatement of the BAM record format and the BGZF container (include/nvbio_amd.h, "BAM output"), written
from the rules -- the behaviour of the reference's io::BamOutput with the three divergences the header lists -- and not from the kernels.
It reuses sam_cpu's helpers and takes sam_cpu's dicts (refs, records).  The encoder (bam_record / bam_records), bam_header and bgzf_frame
are what the library's bytes are compared with; bam_to_sam is a DECODER written on its own, from the BAM specification, which prints
records as SAM lines, so that the library's bytes can also be checked against sam_cpu's text without passing through the encoder here."""
import struct
import zlib

import numpy as np

import sam_cpu

REG2BIN = 2
BGZF_BLOCK_BYTES = 65280
BGZF_EOF = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
U32 = 0xFFFFFFFF


def reg2bin(beg, end):
    """the SAM specification's reg2bin (section 5.3) of the 0-based half-open interval [beg, end)"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def _i32(v):
    v &= U32
    return v - (1 << 32) if v >= 1 << 31 else v


def seq_and_qual_bytes(rec, i):
    """SEQ (4-bit codes, high nibble first) and QUAL (raw bytes, 0xFF when there are none), in the orientation the SAM text has"""
    b, e = int(rec["read_index"][i]), int(rec["read_index"][i + 1])
    rc = (int(rec["state"][i]) >> 1) & 1
    stored = [int(x) for x in rec["reads"][b:e]]
    quals = [0xFF] * (e - b) if rec.get("quals") is None else [int(x) for x in rec["quals"][b:e]]
    flip = (not rc) if rec.get("reads_reversed", True) else bool(rc)
    if flip:
        stored, quals = stored[::-1], quals[::-1]
    if rc:
        stored = [3 - s if s < 4 else s for s in stored]
    codes = [1 << s if s < 4 else 15 for s in stored] + [0]
    return bytes(codes[k] << 4 | codes[k + 1] for k in range(0, e - b, 2)), bytes(quals)


def bam_record(refs, rec, i, flags=0):
    """the bytes of record i, block_size first, or None for a record that is skipped"""
    st = int(rec["state"][i])
    name = rec["names"][i] + b"\0"
    seq, qual = seq_and_qual_bytes(rec, i)
    rlen = int(rec["read_index"][i + 1]) - int(rec["read_index"][i])
    unmapped_bin = 4680 if flags & REG2BIN else 0

    def record(ref_id, pos, bin_, mapq, flag, cigar, next_ref, next_pos, tlen, tags):
        body = struct.pack("<iiIIIiii", ref_id, pos, bin_ << 16 | mapq << 8 | len(name), flag << 16 | len(cigar), rlen, next_ref, next_pos, tlen)
        body += name + b"".join(struct.pack("<I", c) for c in cigar) + seq + qual + tags
        return struct.pack("<i", len(body)) + body

    if not st & 1:
        return record(-1, -1, unmapped_bin, 0, 4, [], -1, -1, 0, b"")
    els = sam_cpu.cigar_elements(rec, i)
    if els is None or sum(l for l, t in els if t != 2) != rlen:
        return None
    si = refs["sequence_index"]
    pos = int(rec["pos"][i])
    s = sam_cpu.sequence_of(refs, pos)
    flag = (128 if st & 4 else 64) | (16 if st & 2 else 0)
    mate = None if rec.get("mate_of") is None else int(rec["mate_of"][i])
    if mate is not None:
        ms = int(rec["state"][mate])
        flag |= 1 | (2 if ms & 8 else 0) | (0 if ms & 1 else 8) | (32 if ms & 2 else 0)
    ref_len = sam_cpu.reference_length(els)
    if ((pos + ref_len) & U32) > int(si[s + 1]):
        return record(-1, -1, unmapped_bin, 0, flag | 4, [], -1, -1, 0, b"")
    own = _i32(pos - int(si[s]))
    cigar = [l << 4 | (0, 1, 2, 4)[t] for l, t in reversed(els)]
    next_ref, next_pos, tlen = -1, -1, 0
    if mate is not None and int(rec["state"][mate]) & 1:
        mpos = int(rec["pos"][mate])
        ms_ = sam_cpu.sequence_of(refs, mpos)
        mref = sam_cpu.reference_length(sam_cpu.cigar_elements(rec, mate) or [])
        next_ref, next_pos = ms_, _i32(mpos - int(si[ms_]))
        if ms_ == s:
            tlen = _i32(max((mpos + mref) & U32, (pos + ref_len) & U32) - min(mpos, pos))
            if mpos < pos:
                tlen = -tlen
    elif mate is not None:
        next_ref, next_pos = s, own
    md, mm, gapo, gape = sam_cpu.md_and_counts(rec, i)
    tags = b"NMc" + bytes([int(rec["ed"][i]) & 255]) + b"ASi" + struct.pack("<i", int(rec["score"][i]))
    if rec.get("second_score") is not None and int(rec["second_score"][i]) != sam_cpu.SCORE_MIN:
        tags += b"XSi" + struct.pack("<i", int(rec["second_score"][i]))
    tags += b"XMc" + bytes([mm & 255]) + b"XOc" + bytes([gapo & 255]) + b"XGc" + bytes([gape & 255])
    if md:
        tags += b"MDZ" + md.encode("latin-1") + b"\0"
    bin_ = reg2bin(own, own + ref_len) if flags & REG2BIN else 0
    return record(s, own, bin_, int(rec["mapq"][i]), flag, cigar, next_ref, next_pos, tlen, tags)


def bam_records(refs, rec, flags=0):
    """-> (data bytes, offsets int64 [n + 1], n_skipped)"""
    n = len(rec["names"])
    parts = [bam_record(refs, rec, i, flags) for i in range(n)]
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([0 if p is None else len(p) for p in parts]) if n else 0
    return b"".join(p for p in parts if p is not None), offsets, sum(p is None for p in parts)


def bam_header(names, lengths, text=None):
    if text is None:
        text = sam_cpu.sam_header([], [])
    out = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(names))
    for n, l in zip(names, lengths):
        n = n if isinstance(n, bytes) else n.encode("latin-1")
        out += struct.pack("<I", len(n) + 1) + n + b"\0" + struct.pack("<I", int(l))
    return out


def bgzf_frame(data):
    """BGZF blocks of at most 65280 payload bytes, each one stored DEFLATE block: 18 bytes of gzip header, 01 LEN NLEN, the payload,
    CRC32 ISIZE.  No EOF block."""
    out = []
    for at in range(0, len(data), BGZF_BLOCK_BYTES):
        p = data[at:at + BGZF_BLOCK_BYTES]
        out.append(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", len(p) + 31 - 1))
        out.append(b"\1" + struct.pack("<HH", len(p), len(p) ^ 0xFFFF) + p + struct.pack("<II", zlib.crc32(p) & U32, len(p)))
    return b"".join(out)


def bgzf_blocks(framed):
    """the blocks of a BGZF stream parsed field by field -> [(bsize, len, nlen, payload, crc, isize)]; every fixed byte is asserted"""
    blocks, at = [], 0
    while at < len(framed):
        assert framed[at:at + 16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]), at
        bsize, = struct.unpack_from("<H", framed, at + 16)
        if framed[at + 18] == 3:                                       # the EOF block: an empty fixed-Huffman block
            assert framed[at:at + 28] == BGZF_EOF
            blocks.append((bsize, 0, 0xFFFF, b"", 0, 0))
        else:
            assert framed[at + 18] == 1
            ln, nlen = struct.unpack_from("<HH", framed, at + 19)
            crc, isize = struct.unpack_from("<II", framed, at + 23 + ln)
            blocks.append((bsize, ln, nlen, framed[at + 23:at + 23 + ln], crc, isize))
        at += bsize + 1
    assert at == len(framed)
    return blocks


# ---- the decoder: BAM records -> SAM lines, from the BAM specification (section 4.2) ------------------------------------------------------
def bam_to_sam(data, refs):
    """walks block_size records and prints each as a SAM line (bytes, with the newline).  An absent MD tag prints nothing, 0xFF qualities
    print `*`, the tags print in the record's order with the SAM type of their BAM type (c, i -> i; Z -> Z)."""
    names = [n.decode("latin-1") for n in refs["names"]]
    ref = lambda k: "*" if k < 0 else names[k]
    lines, at = [], 0
    while at < len(data):
        size, = struct.unpack_from("<i", data, at)
        ref_id, pos, bin_mq_nl, flag_nc, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiIIIiii", data, at + 4)
        end, p = at + 4 + size, at + 36
        l_name, mapq, flag, n_cigar = bin_mq_nl & 255, (bin_mq_nl >> 8) & 255, flag_nc >> 16, flag_nc & 0xFFFF
        assert data[p + l_name - 1] == 0
        qname = data[p:p + l_name - 1].decode("latin-1")
        p += l_name
        cigar = "".join("%d%s" % (c >> 4, "MIDNSHP=X"[c & 15]) for c in struct.unpack_from("<%dI" % n_cigar, data, p)) or "*"
        p += 4 * n_cigar
        seq = "".join("=ACMGRSVTWYHKDBN"[data[p + k // 2] >> (0 if k & 1 else 4) & 15] for k in range(l_seq))
        assert l_seq % 2 == 0 or data[p + l_seq // 2] & 15 == 0
        p += (l_seq + 1) // 2
        q = data[p:p + l_seq]
        qual = "*" if l_seq and all(b == 0xFF for b in q) else "".join(chr(b + 33) for b in q)
        p += l_seq
        tags = []
        while p < end:
            tag, typ = data[p:p + 2].decode(), chr(data[p + 2])
            p += 3
            if typ in "cCsSiI":
                fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ]
                tags.append("%s:i:%d" % (tag, struct.unpack_from(fmt, data, p)[0]))
                p += struct.calcsize(fmt)
            else:
                assert typ == "Z"
                z = data.index(b"\0", p)
                tags.append("%s:Z:%s" % (tag, data[p:z].decode("latin-1")))
                p = z + 1
        assert p == end
        rnext = "*" if next_ref < 0 else "=" if next_ref == ref_id else ref(next_ref)
        fields = [qname, str(flag), ref(ref_id), str(pos + 1), str(mapq), cigar, rnext, str(next_pos + 1), str(tlen), seq, qual] + tags
        lines.append(("\t".join(fields) + "\n").encode("latin-1"))
        at = end
    assert at == len(data)
    return lines


def comparable(line):
    """a SAM line (bytes) under the three rules that relate BAM records to the SAM text: an absent MD tag <-> MD:Z:*, and NM / XM / XO / XG
    modulo 256 (the BAM tags have one byte; c is signed, so both sides are reduced); 0xFF qualities <-> `*` is the decoder's own"""
    out = []
    for f in line.rstrip(b"\n").split(b"\t"):
        if f == b"MD:Z:*":
            continue
        if f[:5] in (b"NM:i:", b"XM:i:", b"XO:i:", b"XG:i:"):
            f = f[:5] + b"%d" % (int(f[5:]) & 255)
        out.append(f)
    return b"\t".join(out)
