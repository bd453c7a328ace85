"""CPU-only: the planted lists of tests/record_cases.py reach what they are for -- read off the restatements (tests/sam_cpu.py,
tests/bam_cpu.py), as test_the_257_record_fixture_has_what_it_is_for does for the random fixture -- so that tests/test_gpu_record_edges.py,
which runs the kernels over the same lists, cannot pass by not reaching a path.  Then the restatements themselves where only small numbers
have pinned them: bam_cpu.reg2bin against the definition by containment, and records at large coordinates written out by hand."""
import re
import struct

import numpy as np
import pytest

import bam_cpu
import record_cases as rc
import sam_cpu

KEYS = ("genome", 1, 2, 3, 1000, 1025)


def sam_lines(refs, rec):
    text, _, skipped = sam_cpu.sam_records(refs, rec)
    assert skipped == 0
    return [l.split("\t") for l in text.decode("latin-1").splitlines()]


def bins_of(refs, rec, keep=None):
    """the bins of the records written as mapped (REG2BIN), those of `keep` (a mask) only"""
    data, offsets, _ = bam_cpu.bam_records(refs, rec, bam_cpu.REG2BIN)
    out = []
    for i, o in enumerate(offsets[:-1]):
        flag = int.from_bytes(data[o + 18:o + 20], "little")
        if not flag & 4 and (keep is None or keep[i]):
            out.append(int.from_bytes(data[o + 14:o + 16], "little"))
    return out


def level_of(b):
    """the span (log2) of a bin's level: the bins are numbered level by level, 8^t of them on level t, the coarsest first"""
    return next(29 - 3 * t for t in range(6) if b < (8 ** (t + 1) - 1) // 7)


# ---- the reference tables -----------------------------------------------------------------------------------------------------------
def test_genome_refs_has_what_it_is_for():
    refs = rc.genome_refs()
    si = refs["sequence_index"].astype(np.int64)
    lens, names = np.diff(si), [len(n) for n in refs["names"]]
    assert len(lens) == 10 and si[-1] < 0xC0000000 and (si[:-1] >= 1 << 31).sum() >= 3
    assert (lens == 1 << 29).sum() >= 4 and (lens == 1).sum() == 1 and (lens == 1 << 26).sum() == 1
    assert min(names) == 1 and max(names) == 100 and {63, 64, 65} <= set(names)
    assert lens[np.flatnonzero(si[:-1] >= 1 << 31)[0]] == 1 << 29       # a whole 2^29 sequence lies past 2^31


@pytest.mark.parametrize("k", KEYS[1:])
def test_many_refs_and_the_binary_search(k):
    refs, rec, _ = rc.coordinate_records(k)
    lens = np.diff(refs["sequence_index"].astype(np.int64))
    assert len(lens) == k and (lens >= 50).all() and (k == 1 or (np.diff(lens) != 0).all())
    si = refs["sequence_index"].astype(np.int64)
    pos = set(rec["pos"][(rec["state"] & 1) != 0].astype(np.int64).tolist())
    assert set(si[:-1].tolist()) <= pos and set((si[1:] - 1).tolist()) <= pos       # the first and the last base of every sequence
    assert {sam_cpu.sequence_of(refs, p) for p in pos} == set(range(k))


def test_one_long_ref():
    assert rc.one_long_ref()["sequence_index"].tolist() == [0, 3100000000]


# ---- coordinates --------------------------------------------------------------------------------------------------------------------
def test_every_reg2bin_level_is_reached():
    for paired in (False, True):
        refs, rec, labels = rc.coordinate_records("genome", paired)
        assert {level_of(b) for b in bins_of(refs, rec)} == set(rc.LEVELS), "every level is reached"
        assert 0 in bins_of(refs, rec), "bin 0 is reached"
        others = [not l.startswith("crosses 2^26") for l in labels]
        assert sum(others) <= len(labels) - 4 and 0 not in bins_of(refs, rec, others), "bin 0 is reached by the records that cross 2^26 alone"
        # a crossing record lies one level above the boundary it crosses, one that ends on it stays at the finest
        data, offsets, _ = bam_cpu.bam_records(refs, rec, bam_cpu.REG2BIN)
        for i, l in enumerate(labels):
            m = re.match(r"(crosses|ends on) 2\^(\d+)", l)
            flag = int.from_bytes(data[offsets[i] + 18:offsets[i] + 20], "little")
            if m and not flag & 4:
                assert level_of(int.from_bytes(data[offsets[i] + 14:offsets[i] + 16], "little")) == (int(m.group(2)) + 3 if m.group(1) == "crosses" else 14), l


def test_pos_widths_large_positions_and_tlen():
    widths, tlens = set(), []
    for key in ("genome", "long"):
        for paired in (False, True):
            refs, rec, labels = rc.coordinate_records(key, paired)
            lines = sam_lines(refs, rec)
            mapped = [l for l in lines if len(l) > 11]
            widths |= {len(l[3]) for l in mapped} | {len(l[7]) for l in mapped if l[6] != "*"}
            tlens += [int(l[8]) for l in mapped]
            written_mapped = np.array([len(l) > 11 for l in lines])
            assert (written_mapped & (rec["pos"] >= 1 << 31)).sum() >= (20 if key == "genome" else 8)      # pos >= 2^31, through an int32 tensor
            if paired:
                assert sum(1 for l in lines if len(l) == 11 and int(l[1]) & 4 and int(l[1]) & 1) >= 4      # bridges keep their pair flags
                assert key == "long" or sum(1 for l in mapped if l[6] not in ("=", "*")) >= 4      # mates on different sequences
                assert sum(1 for l in mapped if int(l[1]) & 8) >= 4                                # a mate unaligned
                assert sum(1 for l in mapped if l[6] == "=" and int(l[7]) > int(l[3])) >= 4 and sum(1 for l in mapped if l[6] == "=" and int(l[7]) < int(l[3])) >= 4
            if key == "long" and paired:                                # a span past 2^31 prints wrapped: the mate in front gets a negative TLEN
                wrapped = [l for l in mapped if l[6] == "=" and int(l[7]) - int(l[3]) > 1 << 31]
                assert len(wrapped) >= 2 and all(1 <= int(l[8]) + (1 << 32) - (int(l[7]) - int(l[3])) <= 10 for l in wrapped)      # + the mate's span
                assert any(int(l[8]) == (1 << 31) - 1 for l in mapped) and any(int(l[8]) == -((1 << 31) - 1) for l in mapped)
            if key == "genome" and paired:
                assert {1 << 29, -(1 << 29), 99999999, -99999999, 100000000, -100000000} <= set(tlens)     # mates 2^29 - 1 apart; 8 | 9 digits
    assert widths == set(range(1, 11))
    assert any(t >= 10 ** 8 for t in tlens) and any(t <= -10 ** 8 for t in tlens)


def test_the_largest_position_sums():
    """pos + ref_len (and so mpos + mref of the mate's record) reaches the end of the 3.1 Gbp sequence exactly and passes it; on the genome
    it reaches and passes the end of the last sequence, past 2^31"""
    for key, top in (("long", 3100000000), ("genome", 2760864386)):
        refs, rec, _ = rc.coordinate_records(key, True)
        aligned = np.flatnonzero(rec["state"] & 1)
        sums = {int(rec["pos"][i]) + sam_cpu.reference_length(sam_cpu.cigar_elements(rec, i)) for i in aligned}
        assert top in sums and max(sums) > top > 1 << 31 and max(sums) < 1 << 32


# ---- classes ------------------------------------------------------------------------------------------------------------------------
def test_the_formulas_on_the_checked_examples():
    assert [rc.bam_need(*a) for a in ((20, 4, 100, None), (40, 8, 300, None), (40, 1024, 300, 320), (40, 3000, 300, 320))] == [274, 610, 5650, 13554]
    assert [rc.sam_need(*a) for a in ((20, 5, 4, 100, None), (40, 16, 700, 300, 320), (40, 16, 2000, 300, 320))] == [463, 6056, 13856]
    assert rc.bam_need(40, 3955, 150, 64) == 16381 and rc.bam_need(40, 3956, 150, 64) == 16385      # the boundary tests/test_bam_abi.py pins


@pytest.mark.parametrize("fmt", ["sam", "bam"])
def test_every_class_is_hit_exactly(fmt):
    classes = rc.SAM_CLASSES if fmt == "sam" else rc.BAM_CLASSES
    shapes = rc.class_shapes(fmt)
    assert {s["cls"] for s in shapes} == set(classes) | {0}
    for k, c in enumerate(classes):
        inside, last, first = shapes[3 * k:3 * k + 3]
        lower = classes[k - 1] if k else 0
        assert lower < inside["need"] < c and inside["cls"] == c
        assert last["need"] == c and last["cls"] == c
        assert first["need"] == c + 1 and first["cls"] == (classes[k + 1] if k + 1 < len(classes) else 0)
    assert max(s["name"] for s in shapes) == 254 and max(s["cs"] for s in shapes) >= 2000
    groups = {rc.BAM_GROUPS[s["cls"]] for s in shapes if s["cls"]} if fmt == "bam" else {4}
    assert groups == ({16, 8, 4} if fmt == "bam" else {4})


CLASS_CASES = [(fmt, i) for fmt in ("sam", "bam") for i, s in enumerate(rc.class_shapes(fmt)) if s["cls"]]


@pytest.mark.parametrize("fmt,index", CLASS_CASES, ids=["%s-%s" % (f, rc.shape_id(rc.class_shapes(f)[i])) for f, i in CLASS_CASES])
def test_a_class_batch_has_what_it_is_for(fmt, index):
    refs, rec, shape = rc.class_batch(fmt, index)
    n = len(rec["names"])
    assert 33 <= n <= 70 and n % 4 and n % 8 and n % 16               # a full and a short last workgroup of 4, 8 and 16 records
    assert max(len(x) for x in refs["names"]) == shape["ref_name"]
    assert rec["cigars"].shape[1] == shape["cs"] and (None if rec["mds"] is None else rec["mds"].shape[1]) == shape["ms"]
    name_lens, read_lens = [len(x) for x in rec["names"]], np.diff(rec["read_index"].astype(np.int64))
    assert max(name_lens) == shape["name"] and name_lens.count(shape["name"]) >= 3 and read_lens.max() == shape["mrl"] and (read_lens == shape["mrl"]).sum() >= 5
    full = rec["cigar_lens"] == shape["cs"]
    assert full.sum() >= 6
    widths = {len(str(int(l))) for l in (rec["cigars"][full] >> 2).ravel()}
    assert widths >= ({1, 2, 3, 4, 5} if shape["cs"] >= 16 else {1, 5})
    lens = np.array([rc.record_bytes(fmt, refs, rec, i) for i in range(n)])
    offsets = np.concatenate([[0], np.cumsum(lens)])
    assert (lens > 0).all() and set((offsets[:-1] % 16).tolist()) == set(range(16))
    cap = shape["cls"] - rc._stage(shape["ms"])
    assert offsets[rc.NEAR] % 16 == 15 and lens[rc.NEAR] == lens.max() and 15 + lens.max() <= cap      # the longest record, at the worst residue, whole
    assert rec["second_score"][rc.NEAR] != sam_cpu.SCORE_MIN and len(rec["names"][rc.NEAR]) == shape["name"] and read_lens[rc.NEAR] == shape["mrl"]
    if shape["ms"]:
        md = sam_cpu.md_and_counts(rec, rc.NEAR)[0]
        assert rec["mds_lens"][rc.NEAR] > shape["ms"] - 5 and len(md) >= 1.19 * (shape["ms"] - 6)      # 6 characters from every 5 bytes
        assert (rec["mds_lens"] <= shape["ms"]).all()                 # well-formed streams only: the bound holds for them
    if shape["need"] == shape["cls"]:                                 # on the boundary the widest record fills most of the LDS left to it (what is
        assert 15 + lens.max() >= 0.85 * cap                           # left over: the integer fields at their widest, MD at 1.5 against 1.2 a byte)


# ---- TOO_LONG -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["smallest", "largest"])
@pytest.mark.parametrize("fmt", ["sam", "bam"])
def test_the_too_long_batches_overflow_where_they_should(fmt, which):
    refs, rec, shape, cap = rc.too_long_batch(fmt, which)
    n = len(rec["names"])
    lens = np.array([rc.record_bytes(fmt, refs, rec, i) for i in range(n)])
    offsets = np.concatenate([[0], np.cumsum(lens)])
    assert [i for i in range(n) if offsets[i] % 16 + lens[i] > cap] == [rc.LONG_A, rc.LONG_B]
    assert lens[rc.LONG_A] > cap + 100
    assert lens[rc.LONG_B] <= cap < offsets[rc.LONG_B] % 16 + lens[rc.LONG_B]      # too long only from where it starts
    read_lens = np.diff(rec["read_index"].astype(np.int64))
    assert read_lens[rc.LONG_A] > shape["mrl"] and read_lens[rc.LONG_B] > shape["mrl"] and len(rec["names"][rc.LONG_A]) > shape["name"]
    group = 4 if fmt == "sam" else rc.BAM_GROUPS[shape["cls"]]
    assert rc.LONG_A // group == rc.LONG_B // group and rc.LONG_A % group and (rc.LONG_B + 1) % group      # inside one workgroup, not at its ends
    assert shape["cls"] == (rc.SAM_CLASSES if fmt == "sam" else rc.BAM_CLASSES)[0 if which == "smallest" else -1]


# ---- cut MD streams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", rc.CUT_STRIDES)
@pytest.mark.parametrize("fmt", ["sam", "bam"])
def test_the_cut_md_batches(fmt, stride):
    refs, rec, shape, cap = rc.cut_md_batch(fmt, stride)
    n = len(rec["names"])
    assert shape["cls"] == (1024 if fmt == "sam" else 512) and rec["mds"].shape[1] == stride
    assert rc.need_of(fmt, dict(shape, mrl=shape["mrl"] + 2)) > shape["cls"]
    lens = np.array([rc.record_bytes(fmt, refs, rec, i) for i in range(n)])
    offsets = np.concatenate([[0], np.cumsum(lens)])
    over = offsets[:-1] % 16 + lens > cap
    assert over.sum() >= 2 and (~over).sum() >= 10                    # both outcomes
    md = [sam_cpu.md_and_counts(rec, i) for i in range(n)]
    bound = 2 * stride + 16
    assert sum(len(m[0]) > bound and not o for m, o in zip(md, over)) >= 2         # the documented bound fails and the record is still whole
    assert max(len(m[0]) for m in md) >= 257
    ml = rec["mds_lens"]
    assert (ml > stride).sum() >= 4 and (ml == stride).sum() >= 4 and (ml == stride - 1).sum() >= 2
    assert any(m[3] == -1 for m in md)                                # an insertion cut behind its op: XG -1
    texts = {m[0] for m in md}
    assert any(t.endswith("^" + "A" * 255 + "0") for t in texts) and any(t.endswith("^0") for t in texts)
    if stride > 4:
        assert any(re.search(r"\^ACGTA{251}0$", t) for t in texts)        # four bases of the deletion inside the stride, 251 read as 0


# ---- BGZF ---------------------------------------------------------------------------------------------------------------------------
def test_the_bgzf_payloads_reach_every_shift():
    blocks = lambda n: -(-n // 65280)
    assert [rc.bgzf_shift(b) for b in range(16)] == [9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7, 8]
    assert {rc.bgzf_shift(b) for b in range(blocks(5 * 65280 + 33))} == {9, 10, 11, 12, 13, 14}      # what tests/test_gpu_bam.py reaches
    assert {rc.bgzf_shift(b) for n in rc.BGZF_SIZES[:3] for b in range(blocks(n))} == {9, 10, 11, 12, 13, 14, 15, 0, 1}
    assert {rc.bgzf_shift(b) for b in range(blocks(rc.BGZF_SIZES[3]))} == set(range(16))
    assert [n % 65280 for n in rc.BGZF_SIZES] == [1, 0, 4097, 4097] and [blocks(n) for n in rc.BGZF_SIZES] == [8, 8, 9, 17]


# ---- the scan's carry ---------------------------------------------------------------------------------------------------------------
def test_the_scan_batch():
    refs, rec = rc.scan_batch_41()
    lens = np.array([rc.record_bytes("bam", refs, rec, i) for i in range(41)])
    assert len(set(lens.tolist())) >= 6 and not (rec["state"] & 1).any()
    assert (rc.SCAN_N + 1 + 2047) // 2048 == 1026 and rc.SCAN_N % 41


# ---- reg2bin against the definition -------------------------------------------------------------------------------------------------
def reg2bin_by_containment(beg, end):
    """the bin of the deepest level that holds [beg, end) in one bin: level t (0 the coarsest) has 8^t bins of 2^(29 - 3 t) bases, numbered
    from (8^t - 1) / 7"""
    for t in range(5, -1, -1):
        size = 1 << (29 - 3 * t)
        k = beg // size
        if k * size <= beg and end <= (k + 1) * size:
            return (8 ** t - 1) // 7 + k
    raise AssertionError("not inside 2^29")


def test_reg2bin_against_containment():
    rng = np.random.default_rng(5)
    intervals = []
    for s in rc.LEVELS:
        size = 1 << s
        for _ in range(3400):
            m = int(rng.integers(1, (1 << 29) // size + 1))
            near = m * size + int(rng.integers(-3, 4))
            length = int(rng.choice([1, 2, 10, 1000, 1 << 14, (1 << 14) + 1, size, size + 1, int(rng.integers(1, 1 << 20))]))
            beg = near - (length if rng.random() < 0.5 else 0)
            if 0 <= beg and beg + length <= 1 << 29:
                intervals.append((beg, beg + length))
    refs, rec, _ = rc.coordinate_records("genome")
    si = refs["sequence_index"].astype(np.int64)
    for i in np.flatnonzero(rec["state"] & 1):
        own = int(rec["pos"][i]) - int(si[sam_cpu.sequence_of(refs, int(rec["pos"][i]))])
        ref_len = sam_cpu.reference_length(sam_cpu.cigar_elements(rec, i))
        if own + ref_len <= 1 << 29:
            intervals.append((own, own + ref_len))
    assert len(intervals) >= 15000
    seen = set()
    for beg, end in intervals:
        want = reg2bin_by_containment(beg, end)
        assert bam_cpu.reg2bin(beg, end) == want, (beg, end)
        seen.add(level_of(want))
    assert seen == set(rc.LEVELS)


# ---- hand-worked records at large coordinates ---------------------------------------------------------------------------------------
def hand_records(names, reads, state, pos, cigars, mate_of=None):
    n = len(names)
    return dict(names=names, reads=np.concatenate(reads).astype(np.uint8), read_index=np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint32),
                quals=None, state=np.array(state, np.uint8), pos=np.array(pos, np.uint32), score=np.array([-3] * n, np.int32), second_score=None,
                ed=np.array([1] * n, np.uint32), mapq=np.array([42] * n, np.uint8), cigars=np.array(cigars, np.uint16), cigar_lens=np.array([1] * n, np.uint32),
                mds=None, mds_lens=None, mate_of=None if mate_of is None else np.array(mate_of, np.uint32), reads_reversed=True)


def test_hand_worked_sam_records():
    # the last base of sequence 7 of the genome, which starts at 4 x 2^29 + 2^26 + 1000004 = 2215592516: POS 2^29
    refs = rc.genome_refs()
    assert int(refs["sequence_index"][7]) == 2215592516
    rec = hand_records([b"r1"], [[2]], [1], [2215592516 + 536870911], [[1 << 2]])
    name7 = refs["names"][7]
    assert len(name7) == 33
    assert sam_cpu.sam_record(refs, rec, 0) == b"r1\t64\t" + name7 + b"\t536870912\t42\t1M\t*\t0\t0\tG\t*\tNM:i:1\tAS:i:-3\tXM:i:0\tXO:i:0\tXG:i:0\tMD:Z:*\n"
    # one base further is the first base of sequence 8
    rec = hand_records([b"r1"], [[2]], [1], [2215592516 + 536870912], [[1 << 2]])
    assert sam_cpu.sam_record(refs, rec, 0).split(b"\t")[2:4] == [refs["names"][8], b"1"]

    # mates 2,999,999,991 bases apart on the 3.1 Gbp sequence: a at POS 10 (2M, stored reversed: A C prints CA), b at POS 3000000001 (1M, reverse
    # strand: stored T prints A).  The span 3000000001 - 10 + 1 = 2999999992 wraps to 2999999992 - 2^32 = -1294967304 for the mate in front;
    # the mate behind negates it.
    refs = rc.one_long_ref()
    rec = hand_records([b"a", b"b"], [[0, 1], [3]], [1 | 8, 1 | 2 | 4 | 8], [9, 3000000000], [[2 << 2], [1 << 2]], mate_of=[1, 0])
    chrom = refs["names"][0]
    tags = b"\tNM:i:1\tAS:i:-3\tXM:i:0\tXO:i:0\tXG:i:0\tMD:Z:*\n"
    assert sam_cpu.sam_record(refs, rec, 0) == b"a\t99\t" + chrom + b"\t10\t42\t2M\t=\t3000000001\t-1294967304\tCA\t*" + tags
    assert sam_cpu.sam_record(refs, rec, 1) == b"b\t147\t" + chrom + b"\t3000000001\t42\t1M\t=\t10\t1294967304\tA\t*" + tags


def test_hand_worked_bam_records():
    refs = rc.genome_refs()
    start7 = 2215592516
    # 2M over the boundary 7 x 2^26 = 469762048 of sequence 7: own position 469762047, in no bin below the root: bin 0
    rec = hand_records([b"r"], [[0, 3]], [1], [start7 + 469762047], [[2 << 2]])
    want = struct.pack("<iiIIIiii", 7, 469762047, 0 << 16 | 42 << 8 | 2, 64 << 16 | 1, 2, -1, -1, 0) + b"r\0" + struct.pack("<I", 2 << 4) + bytes([0x81, 0xFF, 0xFF])
    want += b"NMc\x01ASi" + struct.pack("<i", -3) + b"XMc\0XOc\0XGc\0"
    assert bam_cpu.bam_record(refs, rec, 0, bam_cpu.REG2BIN) == struct.pack("<i", len(want)) + want
    # 2M ending on 2^26: [67108862, 67108864) stays in the finest bin, 4681 + (67108862 >> 14) = 4681 + 4095 = 8776
    rec = hand_records([b"r"], [[0, 3]], [1], [start7 + 67108862], [[2 << 2]])
    got = bam_cpu.bam_record(refs, rec, 0, bam_cpu.REG2BIN)
    assert struct.unpack_from("<iiI", got, 4) == (7, 67108862, 8776 << 16 | 42 << 8 | 2)
    assert struct.unpack_from("<iiI", bam_cpu.bam_record(refs, rec, 0), 4) == (7, 67108862, 42 << 8 | 2)      # without REG2BIN: 0
    # one base further it crosses: level 2^29 again
    rec = hand_records([b"r"], [[0, 3]], [1], [start7 + 67108863], [[2 << 2]])
    assert struct.unpack_from("<iiI", bam_cpu.bam_record(refs, rec, 0, bam_cpu.REG2BIN), 4) == (7, 67108863, 42 << 8 | 2)
    # mates 2^29 - 1 apart on sequence 7: TLEN +- 2^29
    rec = hand_records([b"a", b"b"], [[0], [3]], [1 | 8, 1 | 4 | 8], [start7, start7 + 536870911], [[1 << 2], [1 << 2]], mate_of=[1, 0])
    a, b = (bam_cpu.bam_record(refs, rec, i, bam_cpu.REG2BIN) for i in (0, 1))
    assert struct.unpack_from("<iiIIIiii", a, 4) == (7, 0, 4681 << 16 | 42 << 8 | 2, (64 | 1 | 2) << 16 | 1, 1, 7, 536870911, 536870912)
    assert struct.unpack_from("<iiIIIiii", b, 4) == (7, 536870911, (4681 + 32767) << 16 | 42 << 8 | 2, (128 | 1 | 2) << 16 | 1, 1, 7, 0, -536870912)
