"""GPU: nvbio_fasta_scan / nvbio_fasta_encode / nvbio_fasta_finish against the CPU restatement (tests/fasta_cpu.py, itself pinned to hand-written
answers by tests/test_fasta_oracle.py), byte for byte: the packed text, both sequence indices, the names, the holes, the per-sequence hole
counts, the frequencies, every chunk's summary and the state behind it.  Every output buffer is pre-filled with 0xAA and is longer than the
capacity handed over: nothing but the arrays' own bytes may change.  Then the refusals, the Python layer and FASTA + FASTQ -> SAM."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import fasta_cpu as fa

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 64
AA32 = np.uint32(0xAAAAAAAA)
STATE_KEYS = ("machine", "n_symbols", "n_seqs", "n_ambs", "n_holes", "n_name_bytes", "last_symbol", "seed", "freq")


def device_parse(amd, chunks, seed=11, caps=None, write=True):
    """the chunks through one state, scan and encode without a synchronisation in between, into guarded buffers sized by upper bounds (or
    caps: words, seqs, names, holes) -> dict of host arrays, `summaries` (one dict per chunk), `states` (one per chunk), `status`"""
    import torch
    total = sum(len(c) for c in chunks)
    cap = dict(words=(total + 15) // 16 + 4, seqs=total + 1, names=total + 1, holes=total + 1)
    cap.update(caps or {})
    aa32 = lambda n: torch.full((n + GUARD,), int(AA32.view(np.int32)), dtype=torch.int32, device="cuda:0")
    aa8 = lambda n: torch.full((n + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
    out = dict(text2=aa32(cap["words"]), seq_offset=aa32(cap["seqs"] + 1), name_index=aa32(cap["seqs"] + 1), names=aa8(cap["names"]),
               hole_offset=aa32(cap["holes"]), hole_rank=aa32(cap["holes"]), hole_amb=aa8(cap["holes"]))
    fin = dict(hole_len=aa32(cap["holes"]), seq_n_ambs=aa32(cap["seqs"]))
    state = amd.fasta_state_init(seed)
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    summaries, states = [], []
    for chunk in chunks:
        t = amd._fastq_text(chunk, "cuda:0")
        summary, temp = amd.fasta_scan(t, state)
        arrays = out if write else {}
        amd.fasta_encode(t, temp, state, status, text2_capacity_words=cap["words"], max_seqs=cap["seqs"], names_capacity=cap["names"], max_holes=cap["holes"],
                         **arrays)
        summaries.append(summary)
        states.append(state.clone())
    if write:
        amd.fasta_finish(state, out["seq_offset"], out["name_index"], out["hole_offset"], out["hole_rank"], fin["hole_len"], fin["seq_n_ambs"],
                         max_seqs=cap["seqs"], max_holes=cap["holes"])
    got = {k: v.cpu().numpy() for k, v in {**out, **fin}.items()}
    for k in got:
        if got[k].dtype == np.int32:
            got[k] = got[k].view(np.uint32)
    got["summaries"] = [amd.fasta_summary(s) for s in summaries]
    got["states"] = [amd.fasta_state(s) for s in states]
    got["final"] = amd.fasta_state(state)
    got["status"] = int(status.item())
    return got


def check(got, want, where=None, summaries=None):
    """the device's arrays are the restatement's, and every byte behind them is still 0xAA"""
    n, nh = want.n_seqs, want.n_holes
    for key, used, fill in (("text2", (want.length + 15) // 16, AA32), ("seq_offset", n + 1, AA32), ("name_index", n + 1, AA32), ("names", len(want.names), 0xAA),
                            ("hole_offset", nh, AA32), ("hole_rank", nh, AA32), ("hole_amb", nh, 0xAA), ("hole_len", nh, AA32), ("seq_n_ambs", n, AA32)):
        assert np.array_equal(got[key][:used], getattr(want, key)), (where, key)
        assert (got[key][used:] == fill).all(), (where, key, "written behind its end")
    f = got["final"]
    assert (f["n_symbols"], f["n_seqs"], f["n_holes"], f["n_ambs"], f["n_name_bytes"]) == (want.length, n, nh, want.n_ambs, len(want.names)), where
    assert f["freq"] == [int(v) for v in want.freq] and f["max_name_len"] == want.max_name_len and f["machine"] == want.machine, where
    assert got["summaries"][-1]["status"] == want.status and got["status"] == 0, where
    if summaries is not None:
        assert got["summaries"] == summaries, (where, got["summaries"], summaries)


def check_chunks(amd, chunks, where=None):
    """device and restatement over the same chunks: the tables, every chunk's summary and the state behind every chunk"""
    p = fa.Parser()
    summaries, states = [], []
    for c in chunks:
        summaries.append(p.feed(c))
        states.append(p.state())
    got = device_parse(amd, chunks)
    check(got, p.finish(), where, summaries)
    for g, w in zip(got["states"], states):
        assert {k: g[k] for k in STATE_KEYS} == w, (where, g, w)
    return got


@pytest.fixture(scope="module")
def known():
    return np.load(os.path.join(GOLDEN, "fasta_known.npz"))


def soup(seed, n, p_ff=0.0):
    """bytes over "> \\n ACGTNnR-\\r\\xff": many short sequences, headers and holes"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"> \nACGTNnR-\r\xff", dtype=np.uint8)
    p = np.array([0.6, 2, 4, 10, 10, 10, 10, 5, 3, 2, 1, 1, p_ff])
    return alphabet[rng.choice(len(alphabet), n, p=p / p.sum())].tobytes()


def body_of(rng, n_symbols, width=60, p_n=0.0):
    """n_symbols of ACGT (N with probability p_n) in lines of `width`"""
    s = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, n_symbols, p=[(1 - p_n) / 4] * 4 + [p_n])].tobytes()
    return b"\n".join(s[i:i + width] for i in range(0, n_symbols, width)) + b"\n"


# ---- the known files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["known", "end", "cut"])
def test_known_files(amd, known, tag, tmp_path):
    text = known[tag + "_text"].tobytes()
    got = check_chunks(amd, [text], tag)
    status, consumed, machine = (int(v) for v in known[tag + "_summary"])
    s = got["summaries"][0]
    assert (s["status"], s["consumed_bytes"], s["machine"]) == (status, consumed, machine)
    n = len(known[tag + "_symbols"])
    assert np.array_equal(fa.unpack2(got["text2"][:(n + 15) // 16], n), known[tag + "_symbols"])
    for k in ("seq_offset", "seq_n_ambs", "names", "name_index", "hole_offset", "hole_len", "hole_amb"):
        assert np.array_equal(got[k][:len(known[tag + "_" + k])], known[tag + "_" + k]), k
    ref = amd.parse_fasta(text)
    assert ref.status == status and ref.length == n and ref.names == fa.parse(text).name_list()
    ref.save(str(tmp_path / "x"))
    want = fa.parse(text).files()
    for ext in ("pac", "ann", "amb"):
        assert (tmp_path / ("x." + ext)).read_bytes() == want[ext], ext


def test_saved_files_equal_the_reference_programs(amd, known, tmp_path):
    """the files the reference program wrote (tests/test_fasta_oracle.py says how they were recorded): byte for byte for the known file
    without its NUL-first record, which meets no departure; the packed text of the known file itself"""
    recorded = lambda tag, ext: open(os.path.join(GOLDEN, "fasta_%s_ref.%s" % (tag, ext)), "rb").read()
    amd.read_fasta(os.path.join(GOLDEN, "fasta_plain.fa"), chunk_bytes=50).save(str(tmp_path / "plain"))
    for ext in ("pac", "ann", "amb"):
        assert (tmp_path / ("plain." + ext)).read_bytes() == recorded("plain", ext), ext
    amd.parse_fasta(known["known_text"].tobytes()).save(str(tmp_path / "known"))
    assert (tmp_path / "known.pac").read_bytes() == recorded("known", "pac")


@pytest.mark.parametrize("text", [b"", b"no record here\nACGT\n", b">", b">\n", b"\xff", b">a\n\xff", b"> \nN", b">x y z\n\n\n  \n"])
def test_small_texts(amd, text):
    check_chunks(amd, [text], text)


@pytest.mark.parametrize("pad", [1, 15, 16, 17, 4095, 4096, 4097])
def test_leading_spaces_change_nothing(amd, known, pad):
    text = known["known_text"].tobytes()
    want = fa.parse(text)
    got = device_parse(amd, [b" " * pad + text])
    check(got, want, pad)
    assert got["summaries"][0]["consumed_bytes"] == pad + len(text)


# ---- the chunk carry ------------------------------------------------------------------------------------------------------------------
def test_every_two_way_cut_of_the_known_file(amd, known):
    text = known["known_text"].tobytes()
    for c in range(len(text) + 1):
        check_chunks(amd, [text[:c], text[c:]], c)
    end = known["end_text"].tobytes()
    for c in range(len(end) + 1):
        check_chunks(amd, [end[:c], end[c:]], ("end", c))


def test_three_tiles_with_random_three_way_cuts(amd, known):
    rng = np.random.default_rng(5)
    text = known["known_text"].tobytes() + b"\n" + soup(1, 6000) + b">long\n" + body_of(rng, 6000, p_n=0.05) + soup(2, 300)
    assert 12 * 1024 <= len(text) <= 13 * 1024
    assert fa.same(fa.parse(text), fa.parse_fast(text)) is None
    for _ in range(20):
        a, b = sorted(int(v) for v in rng.integers(0, len(text) + 1, 2))
        check_chunks(amd, [text[:a], text[a:b], text[b:]], (a, b))


# ---- word and tile seams ----------------------------------------------------------------------------------------------------------------
def test_sequence_lengths_around_words_and_tiles(amd):
    rng = np.random.default_rng(6)
    lengths = [15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 1, 16, 4096]
    text = b"".join(b">s%d\n" % m + body_of(rng, m, width=70, p_n=0.02) for m in lengths)
    want = fa.parse(text)
    assert [int(v) for v in np.diff(want.seq_offset)] == lengths
    check_chunks(amd, [text], "whole")
    one_line = b"".join(b">s%d\n" % m + body_of(rng, m, width=1 << 20) for m in lengths)        # no line breaks: a tile is 4096 symbols
    check_chunks(amd, [one_line], "one line each")


def test_tiles_that_emit_nothing(amd):
    rng = np.random.default_rng(7)
    head = b">a\n" + body_of(rng, 4096 - 3 - 1 + 7, width=1 << 20)[:-1]                          # ends 7 symbols into its second tile
    blank = b"\n" + b" " * 4096 * 2 + b"\n"                                                      # at least one tile of only white space
    text = head + blank + body_of(rng, 100)
    text += b" " * ((4000 - len(text) - 3) % 4096)                                              # the 5000 'h' begin 96 bytes before a tile: one tile is all 'h'
    text += b">b " + b"h" * 5000 + b"\n" + body_of(rng, 50) + b">c\n" + b"N" * 9
    want = fa.parse(text)
    assert want.n_seqs == 3 and int(want.seq_offset[1]) % 16 != 0
    tiles = [text[i:i + 4096] for i in range(0, len(text), 4096)]
    assert any(not t.strip(b" \n") for t in tiles) and any(set(t) == {ord("h")} for t in tiles)
    check_chunks(amd, [text], "whole")
    check_chunks(amd, [text[:5000], text[5000:9000], text[9000:]], "cut")


def test_a_name_cut_by_a_tile_edge_and_by_a_chunk_edge(amd):
    rng = np.random.default_rng(8)
    first = b">first\n" + body_of(rng, 3000, width=50)
    text = first + b" " * (4096 - 5 - len(first)) + b">a_long_name_over_the_edge comment\n" + body_of(rng, 77) + b">last\nAC"
    at = text.index(b">a_long")
    assert at < 4096 < at + 20
    want = fa.parse(text)
    assert want.name_list() == [b"first", b"a_long_name_over_the_edge", b"last"] and want.max_name_len == 25
    check_chunks(amd, [text], "tile edge")
    for c in range(at, at + 30):
        check_chunks(amd, [text[:c], text[c:]], c)


def test_all_ambiguous_body(amd):
    rng = np.random.default_rng(9)
    raw = np.frombuffer(b"NnRYKMSW-\0\r\t", dtype=np.uint8)[rng.choice(12, 100000, p=[0.5, 0.1] + [0.04] * 10)]
    runs = np.repeat(raw[::3], 3)[:100000]                                                      # runs of 3 and more of one byte: holes longer than 1
    body = np.where(rng.random(100000) < 0.5, raw, runs).astype(np.uint8).tobytes()
    text = b">amb\n" + b"\n".join(body[i:i + 80] for i in range(0, len(body), 80)) + b"\n>tail\nNN"
    want = fa.parse_fast(text)
    assert want.n_ambs == 100002 and want.n_holes > 30000 and int(want.hole_len.max()) >= 3
    assert np.array_equal(want.symbols, fa.draws(11, 0, 100002))
    got = device_parse(amd, [text])
    check(got, want)
    assert np.array_equal(fa.unpack2(got["text2"][:(want.length + 15) // 16], want.length), fa.draws(11, 0, 100002))
    other = device_parse(amd, [text], seed=12345)
    assert np.array_equal(fa.unpack2(other["text2"][:(want.length + 15) // 16], want.length), fa.draws(12345, 0, 100002))


def test_more_than_1024_sequences(amd):
    rng = np.random.default_rng(10)
    text = b"".join(b">q%d c\n" % i + body_of(rng, int(rng.integers(0, 40)), width=25, p_n=0.1) for i in range(1100))
    want = fa.parse(text)
    assert want.n_seqs == 1100 and want.name_list()[1024] == b"q1024"
    check_chunks(amd, [text[:7000], text[7000:]], "1100")


# ---- capacities, NULL outputs, refusals ------------------------------------------------------------------------------------------------
def test_capacities_are_respected(amd, known):
    text = known["known_text"].tobytes() + b"\n" + soup(3, 9000)
    want = fa.parse(text)
    full = dict(words=(want.length + 15) // 16, seqs=want.n_seqs, names=len(want.names), holes=want.n_holes)
    check(device_parse(amd, [text], caps=full), want, "exact")
    for key, arrays in (("words", ("text2",)), ("seqs", ("seq_offset", "name_index")), ("names", ("names",)), ("holes", ("hole_offset", "hole_rank", "hole_amb"))):
        for cut in (1, full[key] // 2, full[key]):
            caps = dict(full)
            caps[key] = full[key] - cut
            got = device_parse(amd, [text[:5000], text[5000:]], caps=caps)
            assert got["status"] == fa.STATUS_CAPACITY, (key, cut)
            for a in arrays:
                fill = 0xAA if got[a].dtype == np.uint8 else AA32
                extra = 1 if key == "seqs" else 0                             # entry max_seqs is the closing entry's place: not written when n_seqs > max_seqs
                assert np.array_equal(got[a][:caps[key]], getattr(want, a)[:caps[key]]), (key, cut, a)
                assert (got[a][caps[key]:] == fill).all(), (key, cut, a, "written past its capacity", extra)
            f = got["final"]                                                  # the state advances by the counts all the same
            assert (f["n_symbols"], f["n_seqs"], f["n_holes"], f["n_name_bytes"]) == (want.length, want.n_seqs, want.n_holes, len(want.names))
            for other in {"text2", "seq_offset", "names", "hole_offset"} - set(arrays):
                used = dict(text2=full["words"], seq_offset=want.n_seqs + 1, names=len(want.names), hole_offset=want.n_holes)[other]
                assert np.array_equal(got[other][:used], getattr(want, other)), (key, cut, other)


def test_null_outputs_count_only(amd, known):
    text = known["known_text"].tobytes() + b"\n" + soup(4, 9000)
    chunks = [text[:3333], text[3333:8000], text[8000:]]
    counted, written = device_parse(amd, chunks, write=False), device_parse(amd, chunks)
    assert counted["states"] == written["states"] and counted["final"] == dict(written["final"], max_name_len=0)
    assert counted["summaries"] == written["summaries"] and counted["status"] == 0
    for k in ("text2", "seq_offset", "name_index", "names", "hole_offset", "hole_rank", "hole_amb"):
        assert (counted[k] == (0xAA if counted[k].dtype == np.uint8 else AA32)).all(), k
    want = fa.parse(text)
    assert counted["final"]["freq"] == [int(v) for v in want.freq] and counted["final"]["n_symbols"] == want.length


def test_refusals_before_any_launch(amd):
    import torch
    L = amd.lib()
    t = torch.zeros(4096 + 16, dtype=torch.uint8, device="cuda:0")
    state = amd.fasta_state_init()
    before = state.clone()
    summary = torch.full((8,), 0x55, dtype=torch.int32, device="cuda:0")
    temp, nb = amd._temp_for(L.nvbio_fasta_temp_bytes, 4096, device="cuda:0")
    sp = ctypes.cast(state.data_ptr(), ctypes.POINTER(amd._FastaState))
    up = ctypes.cast(summary.data_ptr(), ctypes.POINTER(amd._FastaSummary))
    stream = amd._stream_ptr(t.device)
    assert L.nvbio_fasta_scan(0, t.data_ptr() + 1, 4096, sp, up, temp.data_ptr(), nb, stream) == 1 and b"16-byte aligned" in L.nvbio_amd_last_error()
    assert L.nvbio_fasta_scan(0, t.data_ptr(), 1 << 32, sp, up, temp.data_ptr(), nb, stream) == 4 and b"4 GiB" in L.nvbio_amd_last_error()
    assert L.nvbio_fasta_scan(0, t.data_ptr(), 4096 * 100, sp, up, temp.data_ptr(), nb, stream) == 1 and b"temp_bytes too small" in L.nvbio_amd_last_error()
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    none = [None] * 2
    assert L.nvbio_fasta_encode(0, t.data_ptr(), 1 << 32, temp.data_ptr(), nb, sp, None, 0, *none, 0, None, 0, None, None, None, 0, status.data_ptr(), stream) == 4
    assert L.nvbio_fasta_encode(0, t.data_ptr() + 1, 4096, temp.data_ptr(), nb, sp, None, 0, *none, 0, None, 0, None, None, None, 0, status.data_ptr(), stream) == 1
    assert L.nvbio_fasta_encode(0, t.data_ptr(), 4096 * 100, temp.data_ptr(), nb, sp, None, 0, *none, 0, None, 0, None, None, None, 0, status.data_ptr(), stream) == 1
    assert L.nvbio_fasta_encode(0, t.data_ptr(), 4096, temp.data_ptr(), nb, sp, t.data_ptr() + 4, 4, *none, 0, None, 0, None, None, None, 0, status.data_ptr(), stream) == 1
    b = ctypes.c_uint64(0)
    assert L.nvbio_fasta_temp_bytes(1 << 32, ctypes.byref(b)) == 4 and L.nvbio_fasta_temp_bytes(16, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(state, before) and (summary == 0x55).all() and int(status.item()) == 0


def test_overflow_32_is_reported_and_nothing_is_written(amd):
    """a state a symbol short of 2^32 (set by hand: no test can afford the text that leads there)"""
    import torch
    state = amd.fasta_state_init()
    v = state.cpu().numpy().view(np.uint32).copy()
    v[0], v[1] = fa.BODY, 0xFFFFFFFE
    state = torch.from_numpy(v.view(np.int32)).cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    text2 = torch.full((GUARD,), int(AA32.view(np.int32)), dtype=torch.int32, device="cuda:0")
    for text, over in ((b"A\n", False), (b"AC", True)):
        st = state.clone()
        t = amd._fastq_text(text, "cuda:0")
        summary, temp = amd.fasta_scan(t, st)
        assert bool(amd.fasta_summary(summary)["status"] & fa.STATUS_OVERFLOW_32) == over
        if over:
            amd.fasta_encode(t, temp, st, status, text2=text2, text2_capacity_words=0)
            assert int(status.item()) == fa.STATUS_OVERFLOW_32 and torch.equal(st, state) and (amd.u32(text2) == AA32).all()


# ---- size ------------------------------------------------------------------------------------------------------------------------------
def test_eight_mib(amd):
    rng = np.random.default_rng(11)
    parts = []
    for i in range(5):
        m = (8 << 20) * 60 // 61 // 5 - 64
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, m)].copy()
        for _ in range(3):
            at, run = int(rng.integers(0, m - 5000)), int(rng.integers(1, 5000))
            s[at:at + run] = ord("N")
        width = np.concatenate([s, np.full(-m % 60, 0x20, np.uint8)]).reshape(-1, 60)
        lines = np.concatenate([width, np.full((len(width), 1), 0x0A, np.uint8)], axis=1).tobytes()
        parts.append(b">chr%d synthetic\n" % (i + 1) + lines)
    text = b"".join(parts)
    assert 8 * 1000 * 1000 < len(text) <= 8 << 20
    want = fa.parse_fast(text)
    assert want.n_seqs == 5 and 5 <= want.n_holes <= 15
    got = device_parse(amd, [text], caps=dict(seqs=64, names=1024, holes=64))
    check(got, want, "8 MiB", [want.summary])


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------
def reference_equals(ref, want):
    assert ref.length == want.length and ref.n_seqs == want.n_seqs and ref.names == want.name_list() and ref.freq == [int(v) for v in want.freq]
    for key, attr in (("text2", "text2"), ("sequence_index", "seq_offset"), ("name_index", "name_index"), ("hole_offset", "hole_offset"), ("hole_len", "hole_len"),
                      ("seq_n_ambs", "seq_n_ambs")):
        assert np.array_equal(getattr(ref, key).cpu().numpy().view(np.uint32), getattr(want, attr)), key
    assert np.array_equal(ref.hole_amb.cpu().numpy(), want.hole_amb) and np.array_equal(ref.names_data.cpu().numpy(), want.names)
    h = ref.holes
    assert np.array_equal(h[0], want.hole_offset) and np.array_equal(h[1], want.hole_len) and np.array_equal(h[2], want.hole_amb)


def test_read_fasta_over_two_files(amd, known, tmp_path):
    a = known["known_text"].tobytes() + b"\n" + soup(12, 7000)
    b = soup(13, 3000) + b">" + b"x" * 1500 + b" a long name\nAC\n>z\n" + b"ACGTN" * 1000
    pa, pb = tmp_path / "a.fa", tmp_path / "b.fa"
    pa.write_bytes(a)
    pb.write_bytes(b)
    want = fa.parse(a + b)
    assert want.n_seqs > 64 and want.n_holes > 64 and len(want.names) > 1024  # past the arrays' first sizes (64, 64, 1024): they grow
    whole = amd.parse_fasta(a + b)
    reference_equals(whole, want)
    for chunk in (1000, 4097, 1 << 20):
        reference_equals(amd.read_fasta([str(pa), str(pb)], chunk_bytes=chunk), want)
    reference_equals(amd.read_fasta(str(pa), chunk_bytes=777), fa.parse(a))
    refs = whole.sam_refs()
    assert refs.names == want.name_list() and np.array_equal(refs.sequence_index_host, want.seq_offset) and refs.max_name_len == want.max_name_len
    pb.write_bytes(b + b"\n>cut in the header")
    with pytest.raises(amd.NvbioError):
        amd.read_fasta([str(pa), str(pb)], chunk_bytes=1000)


def test_fasta_and_fastq_to_sam_end_to_end(amd, tmp_path):
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    rng = np.random.default_rng(14)
    lengths = [20000, 12000, 18000]
    seqs = [rng.integers(0, 4, m).astype(np.uint8) for m in lengths]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    fasta = b"some notes first\n"
    for i, s in enumerate(seqs):
        t = letters[s].tobytes()
        fasta += b">chr%c sequence %d of a test\n" % (b"ABC"[i], i) + b"\n".join(t[k:k + 60] for k in range(0, len(t), 60)) + b"\n"
    path = tmp_path / "ref.fa"
    path.write_bytes(fasta)
    fmi, genome2, genome_len, refs = pipeline.reference_from_fasta(str(path), chunk_bytes=30000, kmer_len=8, sa_int=1)
    assert genome_len == sum(lengths) and refs.names == [b"chrA", b"chrB", b"chrC"]
    R, M = 200, 100
    placed, fastq = [], b""
    for i in range(R):
        s = int(rng.integers(0, 3))
        at = int(rng.integers(16, lengths[s] - M - 16))
        read = seqs[s][at:at + M]
        rc = bool(rng.random() < 0.5)
        if rc:
            read = 3 - read[::-1]
        placed.append((s, at, rc))
        fastq += b"@r%d\n" % i + letters[read].tobytes() + b"\n+\n" + b"I" * M + b"\n"
    text, _, n_skipped, _, batch = pipeline.fastq_to_sam(fmi, genome2, genome_len, fastq, pipeline.SeedExtendParams.end_to_end(), refs)
    fmi.close()
    assert batch.n == R and n_skipped == 0
    lines = text.cpu().numpy().tobytes().split(b"\n")[:-1]
    assert len(lines) == R
    for i, (line, (s, at, rc)) in enumerate(zip(lines, placed)):
        f = line.split(b"\t")
        assert f[0] == b"r%d" % i and f[2] == b"chr" + b"ABC"[s:s + 1] and int(f[3]) == at + 1 and bool(int(f[1]) & 16) == rc and f[5] == b"%dM" % M, (i, f[:6])
    header = pipeline.sam_header(refs).split(b"\n")
    assert [l for l in header if l.startswith(b"@SQ")] == [b"@SQ\tSN:chr%c\tLN:%d" % (b"ABC"[i], lengths[i]) for i in range(3)]
