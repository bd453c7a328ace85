"""GPU: the SAM text of nvbio_sam_record_offsets / nvbio_sam_format against the plain-Python restatement (tests/sam_cpu.py, itself pinned
to hand-written records by tests/test_sam_oracle.py), byte for byte: offsets, text, the count of skipped records, and not one byte
written past the text.  Then the refusals, and reads -> SAM end to end on a small genome, where every mapped line is also checked
against the genome without the restatement."""
import ctypes
import importlib
import re

import numpy as np
import pytest

import sam_cpu

pytestmark = pytest.mark.gpu

GUARD = 64


def upload(amd, refs, rec):
    """the restatement's dicts -> (SamRefs, SamRecords)"""
    r = amd.SamRefs(refs["names"], refs["sequence_index"])
    lens = np.diff(rec["read_index"].astype(np.int64))
    c = amd.SamRecords(rec["names"], sam_cpu.pack4(rec["reads"]), rec["read_index"], int(lens.max()) if len(lens) else 0, rec["state"], rec["pos"],
                       rec["score"], rec["ed"], rec["mapq"], rec["cigars"], rec["cigar_lens"], quals=rec["quals"], second_score=rec["second_score"],
                       mds=rec["mds"], mds_lens=rec["mds_lens"], mate_of=rec["mate_of"], reads_reversed=rec["reads_reversed"])
    return r, c


def format_guarded(amd, r, c, short=0):
    """offsets, then the text into a buffer pre-filled with 0xAA that is GUARD bytes longer than the text; the capacity handed over is the
    text's length minus `short` -> (buffer, offsets, n_skipped, status, total)"""
    import torch
    offsets = amd.sam_record_offsets(r, c)
    total = int(offsets[-1].item())
    buf = torch.full((total + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    n_skipped, status = amd.sam_format(r, c, offsets, buf[:total - short])
    return buf.cpu().numpy(), offsets.cpu().numpy(), n_skipped, status, total


def check_against_restatement(amd, refs, rec):
    want_text, want_offsets, want_skipped = sam_cpu.sam_records(refs, rec)
    r, c = upload(amd, refs, rec)
    buf, offsets, n_skipped, status, total = format_guarded(amd, r, c)
    assert status == 0
    assert np.array_equal(offsets, want_offsets)
    got = buf[:total].tobytes()
    if got != want_text:                                              # name the first record that differs
        for i in range(len(rec["names"])):
            a, b = got[offsets[i]:offsets[i + 1]], want_text[want_offsets[i]:want_offsets[i + 1]]
            assert a == b, (i, a, b)
    assert got == want_text and n_skipped == want_skipped
    assert (buf[total:] == 0xAA).all()
    return want_offsets, want_skipped


@pytest.fixture(scope="module")
def refs():
    return sam_cpu.random_refs()


@pytest.fixture(scope="module")
def fields_257(refs):
    return sam_cpu.random_records(np.random.default_rng(20240611), 257, refs)


def test_the_257_record_fixture_has_what_it_is_for(refs, fields_257):
    """properties of the inputs, read off the arrays and the restatement: no GPU work here"""
    rec = fields_257
    lens = np.diff(rec["read_index"].astype(np.int64))
    assert set(sam_cpu.SPECIAL_LENS) <= set(lens.tolist()) and lens.min() == 1 and lens.max() == 1023
    name_lens = [len(x) for x in rec["names"]]
    assert min(name_lens) == 1 and max(name_lens) == 40
    stride = rec["cigars"].shape[1]
    cl = rec["cigar_lens"]
    assert (cl == stride).sum() >= 10 and (cl == stride + 1).sum() >= 1 and (cl == 0xFFFFFFFF).sum() >= 1
    els = rec["cigars"][cl <= stride]
    assert set((els & 3).ravel().tolist()) == {0, 1, 2, 3}
    assert {len(str(int(l))) for l in (els >> 2).ravel() if l} == {1, 2, 3, 4}
    aligned, rc = (rec["state"] & 1) != 0, (rec["state"] & 2) != 0
    assert (~aligned).sum() >= 20 and (aligned & rc).sum() >= 50 and (aligned & ~rc).sum() >= 50 and (rec["reads"] >= 4).sum() >= 100
    assert rec["score"].min() == -65536 and rec["score"].max() == 2046
    text, offsets, n_skipped = sam_cpu.sam_records(refs, rec)
    assert n_skipped >= 5                                             # truncated CIGARs and wrong sums
    wrong_sum = [i for i in range(257) if aligned[i] and cl[i] <= stride and sam_cpu.sam_record(refs, rec, i) is None]
    assert len(wrong_sum) >= 2
    assert set((offsets[:-1] % 16).tolist()) == set(range(16))       # records start at every residue: heads and tails of every length
    md = [f for l in text.decode("latin-1").splitlines() for f in l.split("\t") if f.startswith("MD:Z:")]
    assert any(m == "MD:Z:*" for m in md)
    assert any(re.search(r"\^[ACGTN]0", m) for m in md) and any(re.search(r"\^[ACGTN]{255}0", m) for m in md)
    assert any(re.search(r"[ACGTN]{2}", m.split("^")[0]) for m in md) and any(m.startswith("MD:Z:517") for m in md)      # 255 + 255 + 7 merged
    assert (rec["mds_lens"] > rec["mds"].shape[1]).sum() >= 1


@pytest.mark.parametrize("quals", [True, False])
def test_fields_257_records(amd, refs, fields_257, quals):
    rec = dict(fields_257)
    if not quals:
        rec["quals"] = None
    check_against_restatement(amd, refs, rec)


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_fields_small_batches(amd, refs, n):
    rec = sam_cpu.random_records(np.random.default_rng(100 + n), n, refs)
    check_against_restatement(amd, refs, rec)


def test_optional_arrays_absent_and_reads_stored_forward(amd, refs, fields_257):
    rec = dict(fields_257, second_score=None, mds=None, mds_lens=None, reads_reversed=False)
    check_against_restatement(amd, refs, rec)


def test_paired_128_pairs(amd, refs):
    rec = sam_cpu.random_records(np.random.default_rng(77), 256, refs, paired=True)
    st, pos, mate = rec["state"].astype(int), rec["pos"].astype(np.int64), rec["mate_of"].astype(int)
    assert np.array_equal(mate, np.arange(256) ^ 1)
    seq = np.array([sam_cpu.sequence_of(refs, int(p)) for p in pos])
    both = ((st & 1) != 0) & ((st[mate] & 1) != 0)
    cases = {"same sequence": both & (seq == seq[mate]), "different sequences": both & (seq != seq[mate]), "mate before": both & (pos[mate] < pos),
             "mate behind": both & (pos[mate] > pos), "mate unaligned": ((st & 1) != 0) & ((st[mate] & 1) == 0),
             "both unaligned": ((st & 1) == 0) & ((st[mate] & 1) == 0), "mate rc": both & ((st[mate] & 2) != 0), "mate paired": both & ((st[mate] & 8) != 0),
             "mate not paired": both & ((st[mate] & 8) == 0), "anchor is read 2": (np.arange(256) % 2 == 0) & ((st & 4) != 0)}
    for name, hit in cases.items():
        assert hit.sum() >= 4, name
    text, _, _ = sam_cpu.sam_records(refs, rec)
    lines = [l.split("\t") for l in text.decode("latin-1").splitlines()]
    assert sum(1 for l in lines if len(l) == 11 and int(l[1]) & 4 and int(l[1]) & 1) >= 4          # straddlers keep their pair flags
    assert sum(1 for l in lines if len(l) > 11 and l[8].startswith("-")) >= 10 and sum(1 for l in lines if len(l) > 11 and l[6] not in "=*") >= 10
    check_against_restatement(amd, refs, rec)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(amd, refs):
    import torch
    rec = sam_cpu.random_records(np.random.default_rng(3), 16, refs)
    r, c = upload(amd, refs, rec)
    L = amd.lib()
    offsets = torch.full((17,), -1, dtype=torch.int64, device="cuda:0")
    tmp = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    words = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    text = torch.full((1 << 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rs = r.c_struct()

    def both(cs, want, msg):
        assert L.nvbio_sam_record_offsets(0, ctypes.byref(rs), ctypes.byref(cs), 0, p(offsets), p(tmp), tmp.numel(), None) == want
        assert msg in L.nvbio_amd_last_error()
        assert L.nvbio_sam_format(0, ctypes.byref(rs), ctypes.byref(cs), 0, p(offsets), p(text), text.numel(), p(words), ctypes.c_void_p(words.data_ptr() + 4),
                                  None) == want
        assert msg in L.nvbio_amd_last_error()

    cs = c.c_struct()
    cs.cigar_stride = 4096                                            # 6 x 4096 bytes of CIGAR text alone: beyond a wave's 16384 bytes of LDS
    both(cs, 4, b"LDS")
    cs = c.c_struct()
    cs.max_name_len = 16000
    both(cs, 4, b"LDS")
    for field in ("names_dev", "reads4_dev", "state_dev", "cigars_dev", "mds_lens_dev"):
        cs = c.c_struct()
        setattr(cs, field, None)
        both(cs, 1, b"invalid argument")
    cs = c.c_struct()
    assert L.nvbio_sam_record_offsets(0, ctypes.byref(rs), ctypes.byref(cs), 0, p(offsets), p(tmp), 8, None) == 1
    assert b"temp_bytes too small" in L.nvbio_amd_last_error()
    torch.cuda.synchronize()
    assert (offsets == -1).all() and (text == 0xAA).all() and (words == 0).all()      # nothing ran


def test_a_text_capacity_one_byte_short_is_refused_on_the_device(amd, refs):
    rec = sam_cpu.random_records(np.random.default_rng(4), 40, refs)
    rec["state"][-1] = 0                                             # the last record is written for sure (an unaligned read is never skipped)
    want_text, want_offsets, _ = sam_cpu.sam_records(refs, rec)
    r, c = upload(amd, refs, rec)
    buf, offsets, _, status, total = format_guarded(amd, r, c, short=1)
    assert status == amd.SAM_STATUS_CAPACITY and total == len(want_text)
    last = int(want_offsets[-2])
    assert buf[:last].tobytes() == want_text[:last]                   # every record that fits is there
    assert (buf[last:] == 0xAA).all()                                 # the one that does not was not started, and the guard bytes are intact


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def e2e_inputs():
    """a genome of two sequences (12 kbp + 8 kbp) and 200 reads of 100 bp: 190 planted (either strand, 0..3 substitutions, every fifth with
    one indel of 1 or 2 bp) and 10 random ones.  On the CPU path (oracle/cpu_pipeline.seed_and_extend_cpu, end-to-end scheme) 190 of the 190
    planted reads reach the threshold and none of the random ones, which is where the cap of 180 below comes from."""
    rng = np.random.default_rng(424242)
    si = np.array([0, 12000, 20000], np.uint32)
    genome = rng.integers(0, 4, 20000).astype(np.uint8)
    M, R = 100, 200
    reads = np.zeros((R, M), np.uint8)
    truth = []
    for i in range(190):
        s = int(rng.integers(0, 2))
        start = int(rng.integers(int(si[s]) + 5, int(si[s + 1]) - M - 8))
        src = genome[start:start + M + 4].copy()
        if i % 5 == 0:
            at, l = int(rng.integers(30, 70)), int(rng.integers(1, 3))
            src = np.concatenate([src[:at], rng.integers(0, 4, l).astype(np.uint8), src[at:]]) if i % 10 == 0 else np.concatenate([src[:at], src[at + l:]])
        read = src[:M].copy()
        for at in rng.choice(M, int(rng.integers(0, 4)), replace=False):
            read[at] = (read[at] + int(rng.integers(1, 4))) & 3
        rc = bool(rng.random() < 0.5)
        reads[i] = (3 - read[::-1]) if rc else read
        truth.append((s, start, rc))
    reads[190:] = rng.integers(0, 4, (10, M))
    names = [b"read%d/%s" % (i, b"p" if i < 190 else b"x") for i in range(R)]
    return si, genome, reads, names, truth


def walk(cigar, read, window):
    """(read symbols consumed, reference symbols consumed, mismatches, inserted, deleted, gap opens) of a forward CIGAR over a read and the genome behind POS"""
    j = k = mm = ins = dele = gaps = 0
    for l, op in [(int(a), b) for a, b in re.findall(r"(\d+)([MIDS])", cigar)]:
        if op == "M":
            mm += int((read[j:j + l] != window[k:k + l]).sum())
            j += l
            k += l
        elif op == "I":
            ins += l; gaps += 1; j += l
        elif op == "D":
            dele += l; gaps += 1; k += l
        else:
            j += l
    return j, k, mm, ins, dele, gaps


def test_reads_to_sam_end_to_end(amd, orc):
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    si, genome, reads, names, truth = e2e_inputs()
    G, (R, M) = len(genome), reads.shape
    genome2 = orc.pack2(genome)
    fmi = amd.FMIndex.build(genome2, G, kmer_len=8, sa_int=1)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    rb = pipeline.ReadBatch(torch.from_numpy(sam_cpu.pack4(reads.reshape(-1)).view(np.int32)).cuda(), R, M)
    refs = amd.SamRefs([b"seqA", b"seqB"], si)
    text, offsets, n_skipped, records = pipeline.align_to_sam(fmi, g_dev, G, rb, pipeline.SeedExtendParams.end_to_end(), names, refs)
    fmi.close()
    got = text.cpu().numpy().tobytes()

    # (a) the text is the restatement's over the arrays the pipeline itself produced
    dl = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)
    rec = dict(names=names, reads=reads.reshape(-1), read_index=dl(records.read_index, np.uint32), quals=None, state=dl(records.state, np.uint8),
               pos=dl(records.pos, np.uint32), score=dl(records.score, np.int32), second_score=dl(records.second_score, np.int32), ed=dl(records.ed, np.uint32),
               mapq=dl(records.mapq, np.uint8), cigars=dl(records.cigars, np.uint16), cigar_lens=dl(records.cigar_lens, np.uint32), mds=dl(records.mds, np.uint8),
               mds_lens=dl(records.mds_lens, np.uint32), mate_of=None, reads_reversed=False)
    want_text, want_offsets, want_skipped = sam_cpu.sam_records(dict(sequence_index=si, names=[b"seqA", b"seqB"]), rec)
    assert got == want_text and np.array_equal(offsets.cpu().numpy(), want_offsets) and n_skipped == want_skipped == 0

    # (b) every mapped line against the reads and the genome, without the restatement
    lines = got.decode("latin-1").splitlines()
    assert len(lines) == R
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    mapped = 0
    for i, line in enumerate(lines):
        f = line.split("\t")
        assert f[0] == names[i].decode()
        flag = int(f[1])
        if flag & 4:
            assert len(f) == 11 and flag == 4
            continue
        mapped += i < 190
        seq = "".join(comp[c] for c in reversed(f[9])) if flag & 16 else f[9]
        assert seq == "".join("ACGT"[s] for s in reads[i]) and f[10] == "*"
        s = [b"seqA", b"seqB"].index(f[2].encode())
        start = int(si[s]) + int(f[3]) - 1
        as_aligned = np.array(["ACGT".index(c) for c in f[9]], np.uint8)
        j, k, mm, ins, dele, gaps = walk(f[5], as_aligned, genome[start:start + 2 * M])
        assert j == M and start + k <= int(si[s + 1])
        tags = dict(t.split(":", 1) for t in f[11:])
        assert int(tags["NM"][2:]) == mm + ins + dele
        assert int(tags["XM"][2:]) == mm and int(tags["XO"][2:]) == gaps and int(tags["XG"][2:]) == ins + dele - gaps
        assert int(tags["AS"][2:]) == -(6 * mm + 5 * gaps + 3 * (ins + dele))      # end-to-end scheme at constant quality: 6 a mismatch, 5 + 3 l a gap of l
        if i < 190:
            ts, tstart, trc = truth[i]
            assert s == ts and abs(start - tstart) <= 8 and bool(flag & 16) == trc
    assert mapped >= 180                                               # of 190 planted reads (the CPU path maps 190: see e2e_inputs)
    assert all(int(l.split("\t")[1]) == 4 for l in lines[190:])       # random reads do not align
