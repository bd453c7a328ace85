"""CPU-only: what ties the plain-Python restatement of the BAM format (tests/bam_cpu.py) to the format itself.
(a) its encoder reproduces tests/golden/bam_known.bin, seven records spelled out by hand as commented hex (tests/golden/make_bam_known.py)
    over the inputs of sam_known.npz;
(b) its decoder, written on its own from the BAM specification, turns the encoder's bytes for all 24 known records into the lines of
    sam_known.txt, under exactly three rules: an absent MD tag <-> MD:Z:*, 0xFF qualities <-> `*`, NM / XM / XO / XG modulo 256;
(c) its BGZF framing inflates with Python's gzip, which accepts stored BGZF blocks plus the EOF block and verifies every CRC, and every
    block's fields are parsed out and checked;
(d) reg2bin against the SAM specification's worked values.
The GPU tests compare the library with the restatement."""
import gzip
import importlib.util
import os
import zlib

import numpy as np
import pytest

import bam_cpu
import sam_cpu
from test_sam_oracle import GOLDEN, known


def _maker():
    spec = importlib.util.spec_from_file_location("make_bam_known", os.path.join(GOLDEN, "make_bam_known.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_encoder_reproduces_the_hand_written_records():
    refs, se, pe, _ = known()
    maker = _maker()
    want = open(os.path.join(GOLDEN, "bam_known.bin"), "rb").read()
    hand = [maker.record_bytes(r) for r in maker.RECORDS]
    assert len(hand) >= 6 and b"".join(hand) == want                  # the committed file is what the commented hex says
    names = [{"se": se, "pe": pe}[which]["names"][i] for which, i in maker.ORDER]
    assert names == [b"r0", b"rcN", b"del", b"straddle", b"pB/1", b"pB/2", b"pC/1"]
    for (which, i), h in zip(maker.ORDER, hand):
        got = bam_cpu.bam_record(refs, {"se": se, "pe": pe}[which], i)
        assert got == h, (which, i, got.hex(" "), h.hex(" "))
        assert int.from_bytes(h[:4], "little") == len(h) - 4


def test_decoder_prints_the_known_sam_lines():
    refs, se, pe, want = known()
    header = sam_cpu.sam_header(refs["names"], np.diff(refs["sequence_index"].astype(np.int64)))
    want_lines = [l + b"\n" for l in want[len(header):].split(b"\n")[:-1]]
    sd, so, sk = bam_cpu.bam_records(refs, se)
    pd, po, pk = bam_cpu.bam_records(refs, pe)
    assert (sk, pk) == (3, 0) and so[8] == so[9] == so[10] == so[11]  # trunc, trunc2, badsum: the records the SAM text skips
    got = bam_cpu.bam_to_sam(sd, refs) + bam_cpu.bam_to_sam(pd, refs)
    assert len(got) == len(want_lines) == 21
    for g, w in zip(got, want_lines):
        assert bam_cpu.comparable(g) == bam_cpu.comparable(w), (g, w)
    by_name = {g.split(b"\t")[0]: g for g in got}
    assert b"MD:Z:" not in by_name[b"nomd"] and b"MD:Z:*" in [l for l in want_lines if l.startswith(b"nomd")][0]
    assert b"MD:Z:300" in by_name[b"run300"]                           # the merged run is not wrapped to 8 bits
    # without qualities the decoder prints `*`, as the SAM text does
    nq = dict(se, quals=None)
    for g, w in zip(bam_cpu.bam_to_sam(bam_cpu.bam_records(refs, nq)[0], refs), [l for l in sam_cpu.sam_records(refs, nq)[0].split(b"\n")[:-1]]):
        assert g.rstrip(b"\n").split(b"\t")[10] == b"*" and bam_cpu.comparable(g) == bam_cpu.comparable(w)


def test_the_one_byte_tags_wrap_and_the_rules_say_so():
    refs, se, _, _ = known()
    rec = dict(se)
    rec["ed"] = rec["ed"].copy()
    rec["ed"][1] = 300                                                 # NM c keeps the low 8 bits: 44
    data, offsets, _ = bam_cpu.bam_records(refs, rec)
    line = bam_cpu.bam_to_sam(data[offsets[1]:offsets[2]], refs)[0]
    assert b"NM:i:44" in line.split(b"\t")
    assert bam_cpu.comparable(line) == bam_cpu.comparable(sam_cpu.sam_record(refs, rec, 1))


@pytest.mark.parametrize("n", [0, 1, 65280, 65281])
def test_bgzf_restatement_inflates_and_its_fields_are_right(n):
    x = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    framed = bam_cpu.bgzf_frame(x)
    assert len(framed) == n + 31 * ((n + 65279) // 65280)
    assert gzip.decompress(framed + bam_cpu.BGZF_EOF) == x
    blocks = bam_cpu.bgzf_blocks(framed + bam_cpu.BGZF_EOF)
    assert len(blocks) == (n + 65279) // 65280 + 1 and blocks[-1] == (27, 0, 0xFFFF, b"", 0, 0)
    for k, (bsize, ln, nlen, payload, crc, isize) in enumerate(blocks[:-1]):
        want = x[65280 * k:65280 * (k + 1)]
        assert payload == want and ln == isize == len(want) and nlen == ln ^ 0xFFFF and bsize == len(want) + 30
        assert crc == zlib.crc32(want)
    if n:                                                              # gzip does verify the CRC: a flipped payload byte is refused
        bad = bytearray(framed)
        bad[23] ^= 1
        with pytest.raises(Exception):
            gzip.decompress(bytes(bad) + bam_cpu.BGZF_EOF)


def test_reg2bin_worked_values():
    for pos in (0, 1, 16383, 16384, 5 * 16384 + 77, (1 << 29) - 150):
        if (pos >> 14) == ((pos + 99) >> 14):
            assert bam_cpu.reg2bin(pos, pos + 100) == 4681 + (pos >> 14)
    assert bam_cpu.reg2bin(0, 100) == 4681 and bam_cpu.reg2bin(16384, 16385) == 4682
    assert bam_cpu.reg2bin(16300, 16400) == 585                        # crosses a 16 kbp boundary inside one 128 kbp bin
    assert bam_cpu.reg2bin(131000, 131100) == 73                       # crosses a 128 kbp boundary inside one 1 Mbp bin
    assert bam_cpu.reg2bin((1 << 20) - 10, (1 << 20) + 10) == 9 and bam_cpu.reg2bin((1 << 23) - 1, (1 << 23) + 1) == 1
    assert bam_cpu.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    assert bam_cpu.reg2bin(-1, 0) == 4680                              # unmapped: pos -1
    refs, se, _, _ = known()
    data, offsets, _ = bam_cpu.bam_records(refs, se, bam_cpu.REG2BIN)
    bins = {se["names"][i]: int.from_bytes(data[offsets[i] + 14:offsets[i] + 16], "little") for i in range(14) if offsets[i + 1] > offsets[i]}
    assert bins[b"r0"] == 4680 and bins[b"straddle"] == 4680 and bins[b"del"] == 4681 and bins[b"rcN"] == 4681
    plain, _, _ = bam_cpu.bam_records(refs, se)
    assert len(plain) == len(data) and all(plain[offsets[i] + 14:offsets[i] + 16] == b"\0\0" for i in range(14) if offsets[i + 1] > offsets[i])
