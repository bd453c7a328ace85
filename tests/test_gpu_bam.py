"""GPU: the BAM records of nvbio_bam_record_offsets / nvbio_bam_format against the plain-Python restatement (tests/bam_cpu.py, itself
pinned to hand-written records and to the SAM text by tests/test_bam_oracle.py), byte for byte: offsets, data, the count of skipped
records, and not one byte written past the data.  The same bytes decoded by bam_cpu.bam_to_sam against sam_cpu's text, which does not
pass through the encoder's restatement.  nvbio_bgzf_frame against bam_cpu.bgzf_frame and Python's gzip.  Then the refusals, and reads
-> BAM file end to end on the small genome of tests/test_gpu_sam.py."""
import ctypes
import gzip
import importlib
import os

import numpy as np
import pytest

import bam_cpu
import sam_cpu
from test_gpu_sam import e2e_inputs, upload

pytestmark = pytest.mark.gpu

GUARD = 64


def format_guarded(amd, r, c, flags=0, short=0):
    """offsets, then the records into a buffer pre-filled with 0xAA that is GUARD bytes longer than the data; the capacity handed over is
    the data's length minus `short` -> (buffer, offsets, n_skipped, status, total)"""
    import torch
    offsets = amd.bam_record_offsets(r, c, flags)
    total = int(offsets[-1].item())
    buf = torch.full((total + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    n_skipped, status = amd.bam_format(r, c, offsets, buf[:total - short], flags)
    return buf.cpu().numpy(), offsets.cpu().numpy(), n_skipped, status, total


def check_against_restatement(amd, refs, rec, flags=0):
    want_data, want_offsets, want_skipped = bam_cpu.bam_records(refs, rec, flags)
    r, c = upload(amd, refs, rec)
    buf, offsets, n_skipped, status, total = format_guarded(amd, r, c, flags)
    assert status == 0
    assert np.array_equal(offsets, want_offsets)
    got = buf[:total].tobytes()
    if got != want_data:                                              # name the first record that differs
        for i in range(len(rec["names"])):
            a, b = got[offsets[i]:offsets[i + 1]], want_data[want_offsets[i]:want_offsets[i + 1]]
            assert a == b, (i, a.hex(" "), b.hex(" "))
    assert got == want_data and n_skipped == want_skipped
    assert (buf[total:] == 0xAA).all()
    # the decoder's view of the library's bytes against the SAM restatement's text, record by record
    lines = bam_cpu.bam_to_sam(got, refs)
    sam = [sam_cpu.sam_record(refs, rec, i) for i in range(len(rec["names"]))]
    sam = [s for s in sam if s is not None]
    assert len(lines) == len(sam)
    for g, w in zip(lines, sam):
        assert bam_cpu.comparable(g) == bam_cpu.comparable(w), (g, w)
    return want_offsets


@pytest.fixture(scope="module")
def refs():
    return sam_cpu.random_refs()


@pytest.fixture(scope="module")
def fields_257(refs):
    return sam_cpu.random_records(np.random.default_rng(20240611), 257, refs)       # the fixture of tests/test_gpu_sam.py: same seed


def test_the_257_record_fixture_has_what_it_is_for(refs, fields_257):
    """properties of the inputs as BAM sees them, read off the restatement: no GPU work here"""
    rec = fields_257
    data, offsets, n_skipped = bam_cpu.bam_records(refs, rec)
    lens = np.diff(rec["read_index"].astype(np.int64))
    assert lens.min() == 1 and lens.max() == 1023 and (lens % 2 == 1).sum() >= 50 and (lens % 8 != 0).sum() >= 100
    assert n_skipped >= 5
    assert set((offsets[:-1] % 16).tolist()) == set(range(16))       # records start at every residue: heads and tails of every length
    assert (rec["ed"] > 255).sum() >= 5                                # NM keeps the low 8 bits
    lines = bam_cpu.bam_to_sam(data, refs)
    assert sum(b"MD:Z:" not in l and b"NM:i:" in l for l in lines) >= 5         # aligned records without an MD tag
    assert sum(b"XS:i:" in l for l in lines) >= 50 and sum(b"XS:i:" not in l and b"NM:i:" in l for l in lines) >= 50
    assert sum(int(l.split(b"\t")[1]) & 4 != 0 and int(l.split(b"\t")[1]) != 4 for l in lines) >= 3      # ends past its sequence: flags kept


@pytest.mark.parametrize("flags", [0, bam_cpu.REG2BIN])
@pytest.mark.parametrize("quals", [True, False])
def test_fields_257_records(amd, refs, fields_257, quals, flags):
    rec = dict(fields_257)
    if not quals:
        rec["quals"] = None
    check_against_restatement(amd, refs, rec, flags)


@pytest.mark.parametrize("flags", [0, bam_cpu.REG2BIN])
@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_fields_small_batches(amd, refs, n, flags):
    rec = sam_cpu.random_records(np.random.default_rng(100 + n), n, refs)
    check_against_restatement(amd, refs, rec, flags)


@pytest.mark.parametrize("flags", [0, bam_cpu.REG2BIN])
def test_optional_arrays_absent_and_reads_stored_forward(amd, refs, fields_257, flags):
    rec = dict(fields_257, second_score=None, mds=None, mds_lens=None, reads_reversed=False)
    check_against_restatement(amd, refs, rec, flags)


@pytest.mark.parametrize("flags", [0, bam_cpu.REG2BIN])
def test_paired_128_pairs(amd, refs, flags):
    rec = sam_cpu.random_records(np.random.default_rng(77), 256, refs, paired=True)      # tests/test_gpu_sam.py asserts what these pairs cover
    check_against_restatement(amd, refs, rec, flags)
    if flags:
        data, offsets, _ = bam_cpu.bam_records(refs, rec, flags)
        bins = {int.from_bytes(data[o + 14:o + 16], "little") for o in offsets[:-1]}
        assert 4680 in bins and len(bins) >= 4 and min(bins - {4680}) >= 585        # unmapped, and bins of the two finest levels


def test_lengths_only(amd, refs, fields_257):
    r, c = upload(amd, refs, fields_257)
    lens = amd.bam_record_offsets(r, c, amd.BAM_LENGTHS_ONLY).cpu().numpy()
    _, want_offsets, _ = bam_cpu.bam_records(refs, fields_257)
    assert np.array_equal(lens[:-1], np.diff(want_offsets)) and lens[-1] == 0


def test_offsets_scan_over_more_than_one_tile(amd, refs):
    """4100 records: three tiles of the 2048-value scan, the last of them short"""
    rec = sam_cpu.random_records(np.random.default_rng(8), 41, refs, special_lens=())
    n = 4100
    tile = lambda a: np.concatenate([a] * 100)
    lens = np.diff(rec["read_index"].astype(np.int64))
    big = dict(rec, names=rec["names"] * 100, reads=tile(rec["reads"]), quals=tile(rec["quals"]),
               read_index=np.concatenate([[0], np.cumsum(tile(lens))]).astype(np.uint32),
               **{k: tile(rec[k]) for k in ("state", "pos", "score", "second_score", "ed", "mapq", "cigars", "cigar_lens", "mds", "mds_lens")})
    one, one_offsets, _ = bam_cpu.bam_records(refs, rec)
    r, c = upload(amd, refs, big)
    offsets = amd.bam_record_offsets(r, c).cpu().numpy()
    want = np.concatenate([[0], np.cumsum(tile(np.diff(one_offsets)))])
    assert len(offsets) == n + 1 and np.array_equal(offsets, want)
    data, _, _ = amd.bam_records(r, c)
    assert data.cpu().numpy().tobytes() == one * 100


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(amd, refs):
    import torch
    rec = sam_cpu.random_records(np.random.default_rng(3), 16, refs)
    r, c = upload(amd, refs, rec)
    L = amd.lib()
    offsets = torch.full((17,), -1, dtype=torch.int64, device="cuda:0")
    tmp = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    words = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    data = torch.full((1 << 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rs = r.c_struct()

    def both(cs, want, msg, flags=0):
        assert L.nvbio_bam_record_offsets(0, ctypes.byref(rs), ctypes.byref(cs), flags, p(offsets), p(tmp), tmp.numel(), None) == want
        assert msg in L.nvbio_amd_last_error()
        assert L.nvbio_bam_format(0, ctypes.byref(rs), ctypes.byref(cs), flags, p(offsets), p(data), data.numel(), p(words), ctypes.c_void_p(words.data_ptr() + 4),
                                  None) == want
        assert msg in L.nvbio_amd_last_error()

    cs = c.c_struct()
    cs.cigar_stride = 4096                                            # 4 x 4096 bytes of CIGAR alone: with the rest beyond a group's 16384 bytes of LDS
    both(cs, 4, b"LDS")
    cs = c.c_struct()
    cs.max_name_len = 255
    both(cs, 4, b"l_read_name")
    cs = c.c_struct()
    cs.cigar_stride = 65536
    both(cs, 4, b"n_cigar_op")
    both(c.c_struct(), 1, b"unknown flags", flags=8)
    for field in ("names_dev", "reads4_dev", "state_dev", "cigars_dev", "mds_lens_dev"):
        cs = c.c_struct()
        setattr(cs, field, None)
        both(cs, 1, b"invalid argument")
    cs = c.c_struct()
    assert L.nvbio_bam_record_offsets(0, ctypes.byref(rs), ctypes.byref(cs), 0, p(offsets), p(tmp), 8, None) == 1
    assert b"temp_bytes too small" in L.nvbio_amd_last_error()
    assert L.nvbio_bam_format(0, ctypes.byref(rs), ctypes.byref(cs), 0, p(offsets), ctypes.c_void_p(data.data_ptr() + 8), 64, p(words),
                              ctypes.c_void_p(words.data_ptr() + 4), None) == 1
    # the framing call: a capacity one byte short, and misaligned pointers
    out = torch.full((1 << 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    assert L.nvbio_bgzf_frame(0, p(data), 1000, p(out), 1030, None) == 1 and b"out_capacity" in L.nvbio_amd_last_error()
    assert L.nvbio_bgzf_frame(0, ctypes.c_void_p(data.data_ptr() + 4), 1000, p(out), 1 << 16, None) == 1
    assert L.nvbio_bgzf_frame(0, p(data), 1000, ctypes.c_void_p(out.data_ptr() + 8), 1 << 15, None) == 1
    assert L.nvbio_bgzf_frame(0, p(data), 0, p(out), 0, None) == 0                                      # nothing to frame: nothing written
    torch.cuda.synchronize()
    assert (offsets == -1).all() and (data == 0xAA).all() and (words == 0).all() and (out == 0xAA).all()      # nothing ran


def test_a_data_capacity_one_byte_short_is_refused_on_the_device(amd, refs):
    rec = sam_cpu.random_records(np.random.default_rng(4), 40, refs)
    rec["state"][-1] = 0                                             # the last record is written for sure (an unaligned read is never skipped)
    want_data, want_offsets, _ = bam_cpu.bam_records(refs, rec)
    r, c = upload(amd, refs, rec)
    buf, offsets, _, status, total = format_guarded(amd, r, c, short=1)
    assert status == amd.BAM_STATUS_CAPACITY and total == len(want_data)
    last = int(want_offsets[-2])
    assert buf[:last].tobytes() == want_data[:last]                   # every record that fits is there
    assert (buf[last:] == 0xAA).all()                                 # the one that does not was not started, and the guard bytes are intact


def test_offsets_of_other_flags_or_records_are_refused_on_the_device(amd, refs):
    import torch
    rec = sam_cpu.random_records(np.random.default_rng(6), 20, refs)
    rec["state"][0] = 0
    r, c = upload(amd, refs, rec)
    offsets = amd.bam_record_offsets(r, c)
    wrong = offsets.clone()
    wrong[1:] += 1                                                    # record 0 is one byte longer than its own length
    buf = torch.full((int(wrong[-1].item()) + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    n_skipped, status = amd.bam_format(r, c, wrong, buf[:int(wrong[-1].item())])
    assert status == amd.BAM_STATUS_OFFSETS
    first = int(wrong[1].item())
    assert (buf[:first] == 0xAA).all() and (buf[int(wrong[-1].item()):] == 0xAA).all()      # record 0 was not written at all


# ---- BGZF ---------------------------------------------------------------------------------------------------------------------------
BGZF_SIZES = [0, 1, 15, 16, 17, 255, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 4097, 5 * 65280 + 33]


def frame_guarded(amd, payload):
    """nvbio_bgzf_frame into a buffer pre-filled with 0xAA that is GUARD bytes longer than the framed bytes -> (framed bytes, guard)"""
    import torch
    L = amd.lib()
    n = len(payload)
    src = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).cuda() if n else torch.empty(0, dtype=torch.uint8, device="cuda:0")
    framed = amd.bgzf_framed_bytes(n)
    out = torch.full((framed + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert L.nvbio_bgzf_frame(0, ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), framed, None) == 0
    got = out.cpu().numpy()
    return got[:framed].tobytes(), got[framed:]


@pytest.mark.parametrize("n", BGZF_SIZES)
def test_bgzf_frame_random_payloads(amd, n):
    payload = np.random.default_rng(1000 + n % 997).integers(0, 256, n, dtype=np.uint8).tobytes()
    got, guard = frame_guarded(amd, payload)
    want = bam_cpu.bgzf_frame(payload)
    if got != want:                                                   # name the first block and field that differ
        for k, (g, w) in enumerate(zip(bam_cpu.bgzf_blocks(got), bam_cpu.bgzf_blocks(want))):
            assert g[:3] == w[:3] and g[3] == w[3] and g[4:] == w[4:], (k, g[:3], w[:3], hex(g[4]), hex(w[4]), g[5], w[5])
    assert got == want and (guard == 0xAA).all()
    assert gzip.decompress(got + bam_cpu.BGZF_EOF) == payload
    assert amd.bgzf_frame(payload).cpu().numpy().tobytes() == want    # the Python call, from bytes


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_bgzf_frame_constant_payloads(amd, fill):
    """all zeros and all ones over two blocks: a wrong initial or final complement, or a wrong shift constant, shows here"""
    payload = bytes([fill]) * 65281
    got, guard = frame_guarded(amd, payload)
    assert got == bam_cpu.bgzf_frame(payload) and (guard == 0xAA).all()
    assert gzip.decompress(got + bam_cpu.BGZF_EOF) == payload


def test_bgzf_frame_of_a_tensor_that_is_not_aligned(amd):
    import torch
    payload = np.random.default_rng(9).integers(0, 256, 70000, dtype=np.uint8)
    t = torch.from_numpy(payload).cuda()
    assert amd.bgzf_frame(t[3:]).cpu().numpy().tobytes() == bam_cpu.bgzf_frame(payload[3:].tobytes())


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_reads_to_bam_file_end_to_end(amd, orc, tmp_path):
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    si, genome, reads, names, _ = e2e_inputs()
    G, (R, M) = len(genome), reads.shape
    genome2 = orc.pack2(genome)
    fmi = amd.FMIndex.build(genome2, G, kmer_len=8, sa_int=1)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    rb = pipeline.ReadBatch(torch.from_numpy(sam_cpu.pack4(reads.reshape(-1)).view(np.int32)).cuda(), R, M)
    refs = amd.SamRefs([b"seqA", b"seqB"], si)
    params = pipeline.SeedExtendParams.end_to_end()
    data, offsets, n_skipped, records = pipeline.align_to_bam(fmi, g_dev, G, rb, params, names, refs)
    text, sam_offsets, sam_skipped, _ = pipeline.align_to_sam(fmi, g_dev, G, rb, params, names, refs)
    fmi.close()
    assert n_skipped == sam_skipped == 0 and offsets.numel() == R + 1 and int(offsets[-1].item()) == data.numel()

    header = pipeline.bam_header(refs, text=pipeline.sam_header(refs))
    path = os.path.join(str(tmp_path), "out.bam")
    pipeline.write_bam(path, header, data)
    raw = open(path, "rb").read()
    assert raw.endswith(amd.BGZF_EOF)
    blocks = bam_cpu.bgzf_blocks(raw)
    assert blocks[0][3] == header and len(blocks) == 1 + (data.numel() + 65279) // 65280 + 1       # the header has its blocks to itself
    inflated = gzip.decompress(raw)
    got = data.cpu().numpy().tobytes()
    assert inflated == header + got
    assert header == bam_cpu.bam_header([b"seqA", b"seqB"], np.diff(si.astype(np.int64)), text=pipeline.sam_header(refs))

    # the records, decoded, are the text align_to_sam gives for the same inputs (whose own test checks every mapped line against the genome
    # and asserts mapped >= 180: the records are the same, so that argument stands here)
    lines = bam_cpu.bam_to_sam(inflated[len(header):], dict(sequence_index=si, names=[b"seqA", b"seqB"]))
    sam_lines = text.cpu().numpy().tobytes().split(b"\n")[:-1]
    assert len(lines) == len(sam_lines) == R
    for g, w in zip(lines, sam_lines):
        assert bam_cpu.comparable(g) == bam_cpu.comparable(w), (g, w)
    assert sum(int(l.split(b"\t")[1]) & 4 == 0 for l in lines[:190]) >= 180
