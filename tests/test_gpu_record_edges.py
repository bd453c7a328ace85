"""GPU: the SAM and BAM record kernels and the BGZF framing over the planted lists of tests/record_cases.py, byte for byte against the
restatements (tests/sam_cpu.py, tests/bam_cpu.py): the paths that the random 257-record fixture of test_gpu_sam.py / test_gpu_bam.py does
not reach.  tests/test_record_cases_oracle.py proves on the CPU that every list reaches what it is here for.

    coordinates   a 2.76 Gbp genome of ten sequences (positions past 2^31 through the int32 pos tensor, every reg2bin level and bin 0,
                  TLEN of nine digits with both signs, reference names past 64 bytes), tables of 1 / 2 / 3 / 1000 / 1025 sequences for the
                  binary search, and one sequence of 3.1 Gbp for 10-digit POS / PNEXT and a TLEN past the int32 wrap (SAM only)
    classes       every LDS class of sam_plan (5) and bam_plan (6) and both sides of every class boundary, with the declared maxima the
                  shape's own; CIGARs of cigar_stride elements (up to 3707: 58 rounds of the 64-lane loop, 232 of the 16-lane one), names of
                  254 bytes, a record at the bound starting at 15 mod 16; BAM's 8192 / 16384 classes launch 8 / 4 records to a workgroup
    TOO_LONG      records longer than the declared maxima allow, in the smallest and the largest class: refused, nothing of them written,
                  their neighbours in the workgroup whole
    cut MD        MDS streams that end inside a token: whole or TOO_LONG as the restated formula predicts
    BGZF          eight, nine and seventeen blocks: all sixteen byte shifts of bgzf_frame_kernel (9 ... 15, 0, 1 ... 8 over blocks 0 ... 15), a last block of
                  one byte, a row remainder in the last block
    scan carry    2,099,205 records: the second round of bam_scan_sums_kernel"""
import gzip

import numpy as np
import pytest

import bam_cpu
import record_cases as rc
import sam_cpu
import test_gpu_bam as tb
import test_gpu_sam as ts
from test_gpu_bam import frame_guarded
from test_gpu_sam import upload

pytestmark = pytest.mark.gpu

FORMATS = ("sam", "bam")


def upload_declared(amd, refs, rec, shape):
    """upload() with the maxima the shape declares in place of the data's"""
    r, c = upload(amd, refs, rec)
    assert c.cigars.shape[1] == shape["cs"] and (c.mds is None) == (shape["ms"] is None) and (c.mds is None or c.mds.shape[1] == shape["ms"])
    assert r.max_name_len == shape["ref_name"]
    c.max_name_len, c.max_read_len = shape["name"], shape["mrl"]
    return r, c


def restated(fmt, refs, rec, flags=0):
    return sam_cpu.sam_records(refs, rec) if fmt == "sam" else bam_cpu.bam_records(refs, rec, flags)


def format_guarded(amd, fmt, r, c, flags=0):
    return ts.format_guarded(amd, r, c) if fmt == "sam" else tb.format_guarded(amd, r, c, flags)


def lengths_only(amd, fmt, r, c, flags=0):
    if fmt == "sam":
        return amd.sam_record_offsets(r, c, amd.SAM_LENGTHS_ONLY).cpu().numpy()
    return amd.bam_record_offsets(r, c, amd.BAM_LENGTHS_ONLY | flags).cpu().numpy()


def check_declared(amd, fmt, refs, rec, shape, flags=0, too_long=()):
    """offsets, LENGTHS_ONLY, bytes, n_skipped, status and guard of one batch under declared maxima; the records in `too_long` are
    expected to be refused: status TOO_LONG, their bytes still 0xAA, every other record the restatement's"""
    want, want_offsets, want_skipped = restated(fmt, refs, rec, flags)
    r, c = upload_declared(amd, refs, rec, shape)
    buf, offsets, n_skipped, status, total = format_guarded(amd, fmt, r, c, flags)
    assert np.array_equal(offsets, want_offsets)
    lens = lengths_only(amd, fmt, r, c, flags)
    assert np.array_equal(lens[:-1], np.diff(want_offsets)) and lens[-1] == 0
    assert status == ((amd.SAM_STATUS_TOO_LONG if fmt == "sam" else amd.BAM_STATUS_TOO_LONG) if len(too_long) else 0)
    for i in range(len(rec["names"])):
        got = buf[offsets[i]:offsets[i + 1]]
        if i in too_long:
            assert len(got) and (got == 0xAA).all(), i
        else:
            a, b = got.tobytes(), want[want_offsets[i]:want_offsets[i + 1]]
            assert a == b, (i, a[:200], b[:200])
    assert n_skipped == want_skipped == 0 and total == len(want)
    assert (buf[total:] == 0xAA).all()
    return buf[:total].tobytes()


# ---- coordinates --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("key", ["genome", 1, 2, 3, 1000, 1025])
def test_coordinates_sam_and_bam(amd, key, paired):
    refs, rec, _ = rc.coordinate_records(key, paired)
    ts.check_against_restatement(amd, refs, rec)
    for flags in (0, bam_cpu.REG2BIN):
        tb.check_against_restatement(amd, refs, rec, flags)             # bytes, then decoded by bam_to_sam against the SAM restatement


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_coordinates_sam_on_one_sequence_of_3_1_gbp(amd, paired):
    refs, rec, _ = rc.coordinate_records("long", paired)
    ts.check_against_restatement(amd, refs, rec)


# ---- classes ------------------------------------------------------------------------------------------------------------------------
CLASS_CASES = [(fmt, i) for fmt in FORMATS for i in range(len(rc.class_shapes(fmt)))]


@pytest.mark.parametrize("fmt,index", CLASS_CASES, ids=["%s-%s" % (f, rc.shape_id(rc.class_shapes(f)[i])) for f, i in CLASS_CASES])
def test_every_lds_class_and_its_boundary(amd, fmt, index):
    shape = rc.class_shapes(fmt)[index]
    if shape["cls"] == 0:                                             # one byte past the largest class: refused before any launch
        refs, rec, _ = rc.class_batch(fmt, index - 1)
        r, c = upload(amd, refs, rec)
        c.max_name_len = shape["name"]
        with pytest.raises(amd.NvbioError) as e:
            (amd.sam_record_offsets if fmt == "sam" else amd.bam_record_offsets)(r, c)
        assert e.value.status == 4 and "LDS" in str(e.value)
        return
    refs, rec, _ = rc.class_batch(fmt, index)
    got = check_declared(amd, fmt, refs, rec, shape, bam_cpu.REG2BIN if fmt == "bam" and index % 2 else 0)
    if fmt == "bam":
        lines = bam_cpu.bam_to_sam(got, refs)
        assert len(lines) == len(rec["names"])
        for i, g in enumerate(lines):
            assert bam_cpu.comparable(g) == bam_cpu.comparable(sam_cpu.sam_record(refs, rec, i)), i


# ---- TOO_LONG -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["smallest", "largest"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_records_longer_than_declared_are_refused_and_their_neighbours_whole(amd, fmt, which):
    refs, rec, shape, cap = rc.too_long_batch(fmt, which)
    longest_read, longest_name = int(np.diff(rec["read_index"].astype(np.int64)).max()), max(len(x) for x in rec["names"])
    assert longest_read == 1023 > shape["mrl"] and longest_name == 254 > shape["name"]          # what the data has, and is not declared
    check_declared(amd, fmt, refs, rec, shape, too_long=(rc.LONG_A, rc.LONG_B))


# ---- MDS streams that end inside a token --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", rc.CUT_STRIDES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_cut_md_streams_are_whole_or_too_long_as_predicted(amd, fmt, stride):
    refs, rec, shape, cap = rc.cut_md_batch(fmt, stride)
    _, offsets, _ = restated(fmt, refs, rec)
    too_long = [i for i in range(len(rec["names"])) if offsets[i] % 16 + offsets[i + 1] - offsets[i] > cap]
    check_declared(amd, fmt, refs, rec, shape, too_long=too_long)


# ---- BGZF ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.BGZF_SIZES)
def test_bgzf_frame_over_every_shift(amd, n):
    payload = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    got, guard = frame_guarded(amd, payload)
    want = bam_cpu.bgzf_frame(payload)
    if got != want:                                                   # name the first block and field that differ
        for k, (g, w) in enumerate(zip(bam_cpu.bgzf_blocks(got), bam_cpu.bgzf_blocks(want))):
            assert g[:3] == w[:3] and g[3] == w[3] and g[4:] == w[4:], (k, g[:3], w[:3], hex(g[4]), hex(w[4]), g[5], w[5])
    assert got == want and (guard == 0xAA).all()
    assert gzip.decompress(got + bam_cpu.BGZF_EOF) == payload


# ---- the scan's carry ---------------------------------------------------------------------------------------------------------------
def test_offsets_scan_carries_past_1024_tiles(amd):
    import torch
    refs, rec = rc.scan_batch_41()
    _, one_offsets, _ = bam_cpu.bam_records(refs, rec)
    n, reps = rc.SCAN_N, -(-rc.SCAN_N // 41)
    tile = lambda a: np.tile(a, reps)[:n]
    name_lens = tile(np.array([len(x) for x in rec["names"]], np.int64))
    read_lens = tile(np.diff(rec["read_index"].astype(np.int64)))
    assert np.array_equal(tile(np.diff(one_offsets)), 36 + name_lens + 1 + (read_lens + 1) // 2 + read_lens)      # an unaligned record
    want = np.concatenate([[0], np.cumsum(tile(np.diff(one_offsets)))])
    name_index = np.concatenate([[0], np.cumsum(name_lens)]).astype(np.int32)
    read_index = np.concatenate([[0], np.cumsum(read_lens)])
    dev = lambda a: torch.from_numpy(a).cuda()
    names = (dev(np.full(int(name_index[-1]), ord("q"), np.uint8)), dev(name_index), int(name_lens.max()))
    zeros = lambda dt: np.zeros(n, dt)
    c = amd.SamRecords(names, np.zeros(int(read_index[-1]) // 8 + 1, np.uint32), read_index.astype(np.uint32), int(read_lens.max()), zeros(np.uint8), zeros(np.uint32),
                       zeros(np.int32), zeros(np.uint32), zeros(np.uint8), np.zeros((n, 1), np.uint16), zeros(np.uint32))
    r = amd.SamRefs(refs["names"], refs["sequence_index"])
    assert c.n == n and (n + 1 + 2047) // 2048 == 1026
    offsets = amd.bam_record_offsets(r, c).cpu().numpy()
    assert np.array_equal(offsets, want)
    lens = amd.bam_record_offsets(r, c, amd.BAM_LENGTHS_ONLY).cpu().numpy()
    assert np.array_equal(lens[:-1], np.diff(want)) and lens[-1] == 0
