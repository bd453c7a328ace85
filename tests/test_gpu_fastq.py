"""GPU: nvbio_fastq_scan / nvbio_fastq_encode against the CPU restatement (tests/fastq_cpu.py, itself pinned to hand-written answers by
tests/test_fastq_oracle.py), byte for byte: both index arrays, the 4-bit words, the qualities, the names and every field of the summary.
Every output buffer is pre-filled with 0xAA and is longer than the capacity handed over: nothing but the arrays' own bytes may change.
Then the refusals, and FASTQ text -> SAM text end to end."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import fastq_cpu as fc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 64
AA32 = np.uint32(0xAAAAAAAA)
U = fc.UNLIMITED


def device_parse(amd, text, encoding=fc.PHRED33, strand_op=fc.NO_OP, truncate_len=U, max_records=U, words_cap=None, names_cap=None):
    """scan and encode without a synchronisation in between, into guarded buffers sized by the upper bounds (or the given capacities)
    -> dict of host arrays, `summary` (dict) and `status` (encode's word)"""
    import torch
    nb = len(text)
    t = amd._fastq_text(text, "cuda:0")
    p = amd._FastqParams(encoding, strand_op, truncate_len, max_records)
    summary, temp = amd.fastq_scan(t, p)
    words_cap = (nb + 7) // 8 if words_cap is None else words_cap
    names_cap = nb if names_cap is None else names_cap
    n_cap = min(max_records, nb // 5) + 1
    aa32 = lambda n: torch.full((n + GUARD,), int(AA32.view(np.int32)), dtype=torch.int32, device="cuda:0")
    aa8 = lambda n: torch.full((n + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    out = dict(reads4=aa32(words_cap), quals=aa8(8 * words_cap), names=aa8(names_cap), read_index=aa32(n_cap), name_index=aa32(n_cap))
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    amd.fastq_encode(t, p, temp, out["reads4"], out["read_index"], out["quals"], out["names"], out["name_index"], status,
                     reads4_capacity_words=words_cap, names_capacity=names_cap)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("reads4", "read_index", "name_index"):
        got[k] = got[k].view(np.uint32)
    got["summary"] = amd.fastq_summary(summary)
    got["status"] = int(status.item())
    return got


def check(got, want, where=None):
    """the device's arrays are the restatement's, and every byte behind them is still 0xAA"""
    assert got["summary"] == want.summary, (where, got["summary"], want.summary)
    n, ns, nn = want.summary["n_records"], want.summary["n_symbols"], want.summary["n_name_bytes"]
    words = (ns + 7) // 8
    for key, used, fill in (("read_index", n + 1, AA32), ("name_index", n + 1, AA32), ("reads4", words, AA32), ("quals", ns, 0xAA), ("names", nn, 0xAA)):
        assert np.array_equal(got[key][:used], getattr(want, key)), (where, key)
        assert (got[key][used:] == fill).all(), (where, key, "written behind its end")
    assert got["status"] == 0, where


@pytest.fixture(scope="module")
def known():
    return np.load(os.path.join(GOLDEN, "fastq_known.npz"))


@pytest.fixture(scope="module")
def body(known):
    """the known file, its last record ended, and 40 structured random records: lengths 1..40, many reads share words, some over several lines"""
    return known["known_text"].tobytes() + b"\n" + fc.random_records(np.random.default_rng(20250101), 40)


@pytest.mark.parametrize("tag", ["known", "marker"])
def test_known_files(amd, known, tag):
    text = known[tag + "_text"].tobytes()
    for op in range(4):
        check(device_parse(amd, text, fc.PHRED33, op, 4), fc.parse(text, fc.PHRED33, op, 4), op)
    got = device_parse(amd, text, fc.PHRED)
    ri = known[tag + "_read_index"]
    assert np.array_equal(got["read_index"][:len(ri)], ri) and np.array_equal(got["quals"][:ri[-1]], known[tag + "_quals"])
    assert np.array_equal(fc.unpack4(got["reads4"], ri[-1]), known[tag + "_symbols"]) and np.array_equal(got["names"][:len(known[tag + "_names"])], known[tag + "_names"])


@pytest.mark.parametrize("text", [b"", b" \n\n  \n ", b"@one\nACGTN\n+\nIIIII\n", b"@x\0A\0\0I\0", b"@a\nAC\n+\nII", b"@", b"\n@"])
def test_empty_and_single_record_texts(amd, text):
    check(device_parse(amd, text), fc.parse(text))


def test_boundary_sweep(amd, body):
    """k spaces in front of the body, k over 0..272 and around every power of two from 512 to 65536: every field boundary, every quality
    line that begins with '@' and every shared word crosses every lane, wave, workgroup and tile boundary of the launch shapes"""
    want = fc.parse(body, fc.PHRED33, fc.REVERSE_OP)
    assert want.n == 60 and want.summary["status"] == fc.STATUS_LENGTH | fc.STATUS_EMPTY
    ks = list(range(273)) + [b + d for b in (1 << e for e in range(9, 17)) for d in range(-2, 3)]
    for k in ks:
        check(device_parse(amd, b" " * k + body, fc.PHRED33, fc.REVERSE_OP), fc.shifted(want, k), k)


def test_chunking(amd):
    """a ~6 KB file cut at every offset of a 700-byte window: the first part, then its unconsumed tail and the rest"""
    rng = np.random.default_rng(77)
    text = fc.random_records(rng, 90, min_len=10, max_len=40)
    assert 5000 < len(text) < 8000
    whole = fc.parse(text)
    starts = [i for i in range(len(text)) if text[i:i + 1] == b"@" and (i == 0 or text[i - 1:i] == b"\n")]
    assert sum(660 <= s < 1360 for s in starts) >= 3                             # two whole records inside the window, and offset 1024
    for cut in range(660, 1360):
        a, want_a = device_parse(amd, text[:cut]), fc.parse(text[:cut])
        check(a, want_a, cut)
        used = a["summary"]["consumed_bytes"]
        b = device_parse(amd, text[used:])
        assert a["summary"]["n_records"] + b["summary"]["n_records"] == whole.n and b["summary"]["status"] == 0 and b["summary"]["consumed_bytes"] == len(text) - used
        na, nb = a["summary"]["n_symbols"], b["summary"]["n_symbols"]
        assert np.array_equal(np.concatenate([a["quals"][:na], b["quals"][:nb]]), whole.quals), cut
        syms = np.concatenate([fc.unpack4(a["reads4"], na), fc.unpack4(b["reads4"], nb)])
        assert np.array_equal(fc.pack4(syms), whole.reads4), cut
        ma, mb = a["summary"]["n_name_bytes"], b["summary"]["n_name_bytes"]
        assert np.array_equal(np.concatenate([a["names"][:ma], b["names"][:mb]]), whole.names), cut
        ra, rb = a["read_index"][:a["summary"]["n_records"] + 1], b["read_index"][1:b["summary"]["n_records"] + 1]
        assert np.array_equal(np.concatenate([ra, rb + ra[-1]]), whole.read_index), cut


def test_record_cap(amd, body):
    n = fc.parse(body).n
    for cap in (0, 1, n - 1, n, n + 1):
        got, want = device_parse(amd, body, max_records=cap), fc.parse(body, max_records=cap)
        check(got, want, cap)
        assert got["summary"]["n_records"] == min(cap, n)
        rest = body[got["summary"]["consumed_bytes"]:]                            # parsing on from there yields the rest
        more = device_parse(amd, rest)
        check(more, fc.parse(rest), cap)
        assert got["summary"]["n_records"] + more["summary"]["n_records"] == n


def test_parameter_sweep(amd, body):
    every = b"@every\n" + bytes(range(0x21, 0x2B)) + b"\n" + bytes(range(0x2C, 0x7F)) + b"\n+\n" + bytes(c for c in range(1, 256) if c != 10) + b"\n"
    long_read = b"@long\n" + b"ACGTNacgt-" * 230 + b"\n+\n" + b"5" * 2300 + b"\n"    # more than two LDS windows of symbols
    texts = [body, every + b"@z\nAC\n+\n\0" + every + long_read + every]
    assert fc.parse(texts[1]).n == 5
    for text in texts:
        for op in range(4):
            for enc in range(4):
                for trunc in (1, 7, 8, 9, U):
                    check(device_parse(amd, text, enc, op, trunc), fc.parse(text, enc, op, trunc), (op, enc, trunc))


def test_marker_errors(amd, body):
    rng = np.random.default_rng(5)
    head = fc.random_records(rng, 7)
    for text in (b"x" + body, b"\0" + body, b"+@a\nA\n+\nI\n", head + b"\r\n" + body, head + b"ACGT\n" + body, head + b" " * 4096 + b"N" + body,
                 head + b" " * (8192 - len(head)) + b"?" + body, head + b"\n" * (4096 - len(head)) + b"+"):
        got, want = device_parse(amd, text), fc.parse(text)
        check(got, want)
        s = got["summary"]
        assert s["status"] & fc.STATUS_MARKER and s["error_char"] == text[s["error_offset"]] and s["consumed_bytes"] == s["error_offset"]
        assert s["n_records"] == (0 if text[:1] in (b"x", b"\0", b"+") else 7)


def test_length_and_empty_records(amd):
    good = b"@g\nACGT\n+\nIIII\n"
    for text, status, bad in ((good * 3 + b"@s\nACGT\n+\nII\n" + good, fc.STATUS_LENGTH, 3), (good + b"@l\nAC\n+\nIIIII\n" + good, fc.STATUS_LENGTH, 1),
                              (good * 2 + b"@e\n\n+\n\n" + good, fc.STATUS_EMPTY, 2), (b"@e\nAC\n+\n\n" + good + b"@s\nA\n+\nII\n", fc.STATUS_LENGTH | fc.STATUS_EMPTY, 0),
                              (b"@crlf\r\nACGT\r\n+\r\nIIII\r\n" + good, fc.STATUS_LENGTH, 0)):
        got = device_parse(amd, text)
        check(got, fc.parse(text))
        assert got["summary"]["status"] == status and got["summary"]["first_bad_record"] == bad


def test_refusals_before_any_launch(amd):
    import torch
    L = amd.lib()
    text = amd._fastq_text(b"@a\nACGT\n+\nIIII\n", "cuda:0")
    p = amd._FastqParams(fc.PHRED33, fc.NO_OP, U, U)
    summary = torch.full((10,), 0x55, dtype=torch.int32, device="cuda:0")
    temp, nb = amd._temp_for(L.nvbio_fastq_temp_bytes, text.numel(), U, device="cuda:0")
    sp = ctypes.cast(summary.data_ptr(), ctypes.POINTER(amd._FastqSummary))
    scan = lambda params, text_bytes, temp_bytes: L.nvbio_fastq_scan(0, amd._ptr(text), text_bytes, ctypes.byref(params), sp, amd._ptr(temp), temp_bytes, None)
    out = torch.full((64,), 0x55, dtype=torch.int32, device="cuda:0")
    encode = lambda params, text_bytes, temp_bytes: L.nvbio_fastq_encode(0, amd._ptr(text), text_bytes, ctypes.byref(params), amd._ptr(temp), temp_bytes,
                                                                          amd._ptr(out), 4, amd._ptr(out[8:]), amd._ptr(out[16:]), amd._ptr(out[24:]), 16,
                                                                          amd._ptr(out[32:]), amd._ptr(out[40:]), None)
    for call in (scan, encode):
        assert call(p, text.numel(), nb - 257) == 1 and "temp_bytes" in L.nvbio_amd_last_error().decode()
        assert call(amd._FastqParams(4, fc.NO_OP, U, U), text.numel(), nb) == 1 and "quality_encoding" in L.nvbio_amd_last_error().decode()
        assert call(amd._FastqParams(fc.PHRED33, 4, U, U), text.numel(), nb) == 1 and "strand_op" in L.nvbio_amd_last_error().decode()
        assert call(p, 1 << 32, nb) == 4 and "4 GiB" in L.nvbio_amd_last_error().decode()          # UNSUPPORTED, and the small buffer is not touched
    b = ctypes.c_uint64(0)
    assert L.nvbio_fastq_temp_bytes(1 << 32, U, ctypes.byref(b)) == 4
    size = lambda text_bytes, max_records: (L.nvbio_fastq_temp_bytes(text_bytes, max_records, ctypes.byref(b)), b.value)[1]
    assert 256 <= size(0, U) < size(326_000_000, 1_000_000) < 326_000_000 // 4096 * 8 + 1_000_001 * 20 + (1 << 20)   # 8 bytes a tile, 20 a record, the scan's
    assert size(326_000_000, U) > 326_000_000 // 5 * 20 and size((1 << 32) - 1, 1) > 0
    torch.cuda.synchronize()
    assert (summary == 0x55).all() and (out == 0x55).all()


def test_capacity_refusal_on_the_device(amd, body):
    """one word, then one name byte, short: the records that fit are written as ever, the others not at all, the guard bytes stay"""
    want = fc.parse(body)
    ns, nn, n = want.summary["n_symbols"], want.summary["n_name_bytes"], want.n
    words = (ns + 7) // 8
    ri, ni = want.read_index.astype(np.int64), want.name_index.astype(np.int64)
    all_syms = fc.unpack4(want.reads4, ns)
    for words_cap, names_cap in ((words - 1, nn), (words, nn - 1)):
        got = device_parse(amd, body, words_cap=words_cap, names_cap=names_cap)
        assert got["status"] == fc.STATUS_CAPACITY and got["summary"] == want.summary
        assert np.array_equal(got["read_index"][:n + 1], want.read_index) and np.array_equal(got["name_index"][:n + 1], want.name_index)
        fits = (ri[1:] <= 8 * words_cap) & (ni[1:] <= names_cap)
        assert 0 < fits.sum() < n and fits[0]
        syms = np.zeros(8 * min(words, words_cap), np.uint8)
        quals = np.full(len(got["quals"]), 0xAA, np.uint8)
        names = np.full(len(got["names"]), 0xAA, np.uint8)
        for i in np.flatnonzero(fits):
            syms[ri[i]:ri[i + 1]] = all_syms[ri[i]:ri[i + 1]]
            quals[ri[i]:ri[i + 1]] = want.quals[ri[i]:ri[i + 1]]
            names[ni[i]:ni[i + 1]] = want.names[ni[i]:ni[i + 1]]
        assert np.array_equal(got["reads4"][:len(syms) // 8], fc.pack4(syms)) and (got["reads4"][len(syms) // 8:] == AA32).all()
        assert np.array_equal(got["quals"], quals) and np.array_equal(got["names"], names)


def test_size_200k_records_of_150_bp(amd):
    text = fc.uniform_records(np.random.default_rng(1), 200000, 150, name_len=20)
    assert 60e6 < len(text) < 70e6
    check(device_parse(amd, text, fc.PHRED33, fc.REVERSE_OP), fc.parse_fast(text, fc.PHRED33, fc.REVERSE_OP))


def test_parse_fastq_and_read_fastq(amd, body, tmp_path):
    want = fc.parse(body)
    b = amd.parse_fastq(body)
    assert b.n == want.n and b.summary == want.summary and b.status == want.summary["status"]
    for key, dt in (("reads4", np.uint32), ("read_index", np.uint32), ("name_index", np.uint32), ("quals", np.uint8)):
        assert np.array_equal(getattr(b, key).cpu().numpy().view(dt), getattr(want, key)), key
    assert np.array_equal(b.names[0].cpu().numpy(), want.names) and b.names[2] == want.summary["max_name_len"]
    rb = b.read_batch()
    assert rb.n == want.n and rb.read_len == want.summary["max_read_len"] and rb.offsets is b.read_index
    assert amd.parse_fastq(b"@a\nACG\n+\nIII\n@b\nTTT\n+\nIII\n").read_batch().offsets is None
    path = tmp_path / "reads.fq"
    path.write_bytes(body)
    for chunk in (100, 1000, 1 << 20):
        batches = list(amd.read_fastq(str(path), chunk_bytes=chunk))
        assert sum(x.n for x in batches) == want.n
        assert np.array_equal(np.concatenate([x.quals.cpu().numpy() for x in batches]), want.quals)
        assert np.array_equal(np.concatenate([x.names[0].cpu().numpy() for x in batches]), want.names)
    capped = list(amd.read_fastq(str(path), chunk_bytes=1000, max_records=7))
    assert sum(x.n for x in capped) == want.n and max(x.n for x in capped) == 7 and np.array_equal(np.concatenate([x.quals.cpu().numpy() for x in capped]), want.quals)
    path.write_bytes(body + b"@cut\nAC")
    with pytest.raises(amd.NvbioError):
        list(amd.read_fastq(str(path), chunk_bytes=1000))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def e2e_reads(lengths):
    """reads planted in the 20 kbp genome of tests/test_gpu_sam.py (either strand, 0..3 substitutions) and ten random ones"""
    from test_gpu_sam import e2e_inputs
    si, genome, _, _, _ = e2e_inputs()
    rng = np.random.default_rng(99)
    reads = []
    for i, m in enumerate(lengths):
        if i >= len(lengths) - 10:
            reads.append(rng.integers(0, 4, m).astype(np.uint8))
            continue
        s = int(rng.integers(0, 2))
        start = int(rng.integers(int(si[s]) + 5, int(si[s + 1]) - m - 8))
        read = genome[start:start + m].copy()
        for at in rng.choice(m, int(rng.integers(0, 4)), replace=False):
            read[at] = (read[at] + int(rng.integers(1, 4))) & 3
        reads.append((3 - read[::-1]) if rng.random() < 0.5 else read)
    quals = [((np.arange(m) * 7 + i) % 41).astype(np.uint8) for i, m in enumerate(lengths)]
    names = [b"frag%d/1" % i for i in range(len(lengths))]
    return si, genome, reads, quals, names


@pytest.mark.parametrize("ragged", [False, True])
def test_fastq_to_sam_end_to_end(amd, orc, ragged):
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    R = 200
    lengths = [int(l) for l in np.random.default_rng(3).integers(100, 151, R)] if ragged else [150] * R
    si, genome, reads, quals, names = e2e_reads(lengths)
    fastq = b"".join(b"@" + n + b"\n" + bytes(b"ACGT"[s] for s in r) + b"\n+\n" + bytes(q + 33) + b"\n" for n, r, q in zip(names, reads, quals))
    G = len(genome)
    genome2 = orc.pack2(genome)
    fmi = amd.FMIndex.build(genome2, G, kmer_len=8, sa_int=1)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    refs = amd.SamRefs([b"seqA", b"seqB"], si)
    params = pipeline.SeedExtendParams.end_to_end()
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).cuda() if ragged else None
    rb = pipeline.ReadBatch(torch.from_numpy(fc.pack4(np.concatenate(reads)).view(np.int32)).cuda(), R, max(lengths),
                            quals=torch.from_numpy(np.concatenate(quals)).cuda(), offsets=offsets)
    want_text, want_offsets, want_skipped, _ = pipeline.align_to_sam(fmi, g_dev, G, rb, params, names, refs)
    text, sam_offsets, n_skipped, _, batch = pipeline.fastq_to_sam(fmi, g_dev, G, fastq, params, refs)
    fmi.close()
    assert batch.n == R and batch.status == 0 and batch.consumed_bytes == len(fastq)
    got = text.cpu().numpy().tobytes()
    assert got == want_text.cpu().numpy().tobytes() and torch.equal(sam_offsets, want_offsets) and n_skipped == want_skipped
    lines = got.split(b"\n")[:-1]
    assert len(lines) == R
    fq = fastq.split(b"\n")
    unaligned = 0
    for i, line in enumerate(lines):
        f = line.split(b"\t")
        if int(f[1]) == 4:                                                        # unaligned: SEQ and QUAL are the FASTQ lines
            unaligned += 1
            assert f[0] == fq[4 * i][1:] and f[9] == fq[4 * i + 1] and f[10] == fq[4 * i + 3]
    assert 10 <= unaligned < 40
