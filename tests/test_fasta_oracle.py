"""CPU-only: the restatement of the FASTA grammar (tests/fasta_cpu.py) against answers written out by hand (tests/golden/fasta_known.txt),
its generator against libc's drand48, the machine as a composition of per-byte functions against the serial loop, the chunk carry
against the whole parse, and the vectorised path against the serial loop.  The GPU tests compare the library with this restatement
byte for byte."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import fasta_cpu as fa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("known", "end", "cut")


def known():
    return np.load(os.path.join(GOLDEN, "fasta_known.npz"))


def test_the_packed_answers_are_the_files():
    spec = importlib.util.spec_from_file_location("make_fasta_known", os.path.join(GOLDEN, "make_fasta_known.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    packed, z = mod.pack(), known()
    assert sorted(packed) == sorted(z.files)
    for k in packed:
        assert np.array_equal(packed[k], z[k]), k


def test_the_known_files_hold_what_they_are_for():
    z = known()
    text = z["known_text"].tobytes()
    first = text.index(b">")
    names = [z["known_names"].tobytes()[a:b] for a, b in zip(z["known_name_index"][:-1], z["known_name_index"][1:])]
    assert first > 0 and text[:first].strip()                                          # junk before the first '>'
    assert b">seq1 a comment here\n" in text and b">seq2\n" in text                    # a header with a comment and one without
    assert b"NNAC>seq3" in text                                                        # a '>' in mid-body
    assert b"acgt" in text and all(c in text for c in b"RYK")                          # lower case, IUPAC letters
    assert b"NNnN" in text and b"ACNN\nNNAC" in text                                   # N next to n, a hole across a line break
    assert b"ACGN\n>s7\nNNAC" in text                                                  # the same byte ends one sequence and starts the next
    assert all(c in text for c in (b"-", b"\r", b"\t", b"A\0C", b">nulfirst\n\0"))     # '-', CR, tab, a NUL that is not first, one that is
    assert b">empty\n>" in text and b"AC G T" in text and not text.endswith(b"\n")     # an empty sequence, spaces inside lines, no final newline
    assert 0 in z["known_seq_offset"][1:] - z["known_seq_offset"][:-1] and b"empty" in names
    h = {(int(o), int(l), int(a)) for o, l, a in zip(z["known_hole_offset"], z["known_hole_len"], z["known_hole_amb"])}
    assert {(8, 2, ord("N")), (10, 1, ord("n")), (11, 1, ord("N")), (18, 4, ord("N")), (46, 1, ord("N")), (47, 2, ord("N")), (39, 2, 0)} <= h
    end = z["end_text"].tobytes()
    assert 0xFF in end[end.index(b"\n"):] and z["end_summary"][0] == fa.STATUS_END_BYTE and z["end_summary"][1] < len(end)
    assert b"\n" not in z["cut_text"].tobytes()[z["cut_text"].tobytes().rindex(b">"):] and z["cut_summary"][0] == fa.STATUS_INCOMPLETE


def equals_known(r, z, tag):
    assert np.array_equal(r.symbols, z[tag + "_symbols"]) and np.array_equal(r.text2, fa.pack2(z[tag + "_symbols"])), tag
    assert np.array_equal(fa.unpack2(r.text2, r.length), z[tag + "_symbols"]), tag
    for k in ("seq_offset", "seq_n_ambs", "names", "name_index", "hole_offset", "hole_len", "hole_amb"):
        assert np.array_equal(getattr(r, k), z[tag + "_" + k]), (tag, k)
    assert np.array_equal(r.freq, np.bincount(z[tag + "_symbols"], minlength=4)), tag


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_equals_the_hand_written_answers(tag):
    z = known()
    text = z[tag + "_text"].tobytes()
    r = fa.parse(text)
    equals_known(r, z, tag)
    status, consumed, machine = (int(v) for v in z[tag + "_summary"])
    s = r.summary
    assert (s["status"], s["consumed_bytes"], s["machine"]) == (status, consumed, machine)
    assert (s["n_symbols"], s["n_seqs"], s["n_holes"], s["n_ambs"]) == (r.length, r.n_seqs, r.n_holes, int(z[tag + "_ambiguous"].sum()))
    assert s["n_name_bytes"] == len(z[tag + "_names"])
    fast = fa.parse_fast(text)
    assert fa.same(fast, r) is None and fast.summary == r.summary


def test_the_saved_files_by_hand():
    """.pac, .ann and .amb of a text small enough to write out: save_bpac (4 symbols a byte, a 0 byte when the length is a multiple of 4,
    then the length mod 4) and save_bns ("%lld %d %u", "%d %s %s", "%lld %d %d"; "%lld %d %u", "%lld %d %c")"""
    f = fa.parse(b">chr1 human\nACGT\nAC\n>chr2\nTTNNTTGA\n").files()
    d = [int(fa.draw(11, k)) for k in range(2)]
    syms = [0, 1, 2, 3, 0, 1, 3, 3, d[0], d[1], 3, 3, 2, 0]
    by = lambda q: bytes([(q[0] << 6) | (q[1] << 4) | (q[2] << 2) | q[3]])
    assert f["pac"] == by(syms[0:4]) + by(syms[4:8]) + by(syms[8:12]) + by(syms[12:14] + [0, 0]) + bytes([2])
    assert f["ann"] == b"14 2 11\n0 chr1 null\n0 6 0\n0 chr2 null\n6 8 1\n"
    assert f["amb"] == b"14 2 1\n8 2 N\n"
    g = fa.parse(b">s\nACGTACGT").files()
    assert g["pac"] == bytes([0x1B, 0x1B, 0, 0])


NUL_FIRST = b">nulfirst\n\0\0AC\n"


def recorded(tag):
    return {k: open(os.path.join(GOLDEN, "fasta_%s_ref.%s" % (tag, k)), "rb").read() for k in ("pac", "ann", "amb")}


def test_saved_files_equal_the_reference_programs():
    """fasta_known_ref.* and fasta_plain_ref.* are what the reference's own FASTA_inc_reader, nvBWT Writer, save_bns and save_bpac wrote for
    fasta_known.fa and for fasta_plain.fa, which is the known file without its NUL-first record.  The plain file meets no departure: all three
    files are equal byte for byte.  The known file meets departure d alone: the reference adds the two leading NULs of `nulfirst` to the
    hole of the NUL 37 symbols in, in the sequence before; the text (.pac) is the same, and .ann / .amb differ in exactly those lines."""
    text = known()["known_text"].tobytes()
    plain = open(os.path.join(GOLDEN, "fasta_plain.fa"), "rb").read()
    assert text.count(NUL_FIRST) == 1 and plain == text.replace(NUL_FIRST, b"")
    assert fa.parse(plain).files() == recorded("plain")
    ours, theirs = fa.parse(text).files(), recorded("known")
    assert ours["pac"] == theirs["pac"]
    assert ours["ann"].replace(b"0 nulfirst null\n39 4 1\n", b"0 nulfirst null\n39 4 0\n") == theirs["ann"]
    assert ours["amb"].replace(b"51 7 15\n", b"51 7 14\n").replace(b"37 1 \0\n39 2 \0\n", b"37 3 \0\n") == theirs["amb"]
    assert ours["ann"] != theirs["ann"] and ours["amb"] != theirs["amb"]


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def test_draws_are_libc_drand48():
    libc = ctypes.CDLL("libc.so.6")
    libc.drand48.restype = ctypes.c_double
    libc.srand48(11)
    n = 100000
    want = np.array([int(libc.drand48() * 4) & 3 for _ in range(n)], dtype=np.uint8)
    x, got = fa.lcg_seed(11), np.zeros(n, dtype=np.uint8)
    for i in range(n):
        x = fa.lcg_step(x)
        got[i] = x >> 46
    assert np.array_equal(got, want)
    assert np.array_equal(fa.draws(11, 0, n), want) and np.array_equal(fa.draws(11, 777, 1000), want[777:1777])
    assert np.array_equal(known()["draws"], want[:len(known()["draws"])])


def test_jumps_equal_stepping():
    rng = np.random.default_rng(48)
    ranks = np.sort(rng.integers(0, 1 << 32, 1000))
    x0 = fa.lcg_seed(11)
    # stepping to 2^32 is out of reach: step between neighbouring ranks from a jump that is itself checked against stepping below 2^20
    small = np.sort(rng.integers(0, 1 << 20, 200))
    x, at = x0, 0
    for r in small:
        for _ in range(int(r) - at):
            x = fa.lcg_step(x)
        at = int(r)
        assert fa.lcg_jump(x0, at) == x
    # composition: a jump to r equals a jump to q followed by one of r - q, for the 1000 ranks below 2^32, and one more step is one more rank
    prev, xp = 0, x0
    for r in ranks:
        xr = fa.lcg_jump(x0, int(r))
        assert fa.lcg_jump(xp, int(r) - prev) == xr and fa.lcg_step(xr) == fa.lcg_jump(x0, int(r) + 1)
        prev, xp = int(r), xr


# ---- the machine as functions -------------------------------------------------------------------------------------------------------
def serial_states(text, s=fa.PRE):
    out = []
    for c in text:
        out.append(s)
        s = fa.next_state(s, c)
    return out, s


@pytest.mark.parametrize("seed", range(6))
def test_composition_over_random_tilings_equals_the_serial_states(seed):
    rng = np.random.default_rng(seed)
    if seed < 2:
        text = known()["known_text"].tobytes() + known()["end_text"].tobytes()
    else:
        alphabet = np.frombuffer(b"> \nACGNn\r\xff", dtype=np.uint8)
        p = np.array([3, 3, 4, 4, 4, 4, 4, 4, 2, 0.2 if seed < 5 else 0.0])
        text = alphabet[rng.choice(len(alphabet), 600, p=p / p.sum())].tobytes()
    for start in range(5):
        want, final = serial_states(text, start)
        cuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, len(text)), 25, replace=False)), [len(text)]])
        tile_fns = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            f = fa.IDENTITY
            for c in text[a:b]:
                f = fa.compose(f, fa.byte_fn(c))
            tile_fns.append(f)
        prefix = fa.IDENTITY
        for (a, b), f in zip(zip(cuts[:-1], cuts[1:]), tile_fns):
            s = prefix[start]
            assert s == want[a]
            got, _ = serial_states(text[a:b], s)
            assert got == want[a:b]
            prefix = fa.compose(prefix, f)
        assert prefix[start] == final


# ---- the chunk carry ----------------------------------------------------------------------------------------------------------------
def test_every_two_way_cut_and_random_three_way_cuts_equal_the_whole_parse():
    text = known()["known_text"].tobytes()
    whole = fa.parse(text)
    cuts = [(c,) for c in range(len(text) + 1)]
    rng = np.random.default_rng(3)
    cuts += [tuple(sorted(rng.integers(0, len(text) + 1, 2))) for _ in range(200)]
    for cut in cuts:
        edges = [0, *cut, len(text)]
        r = fa.parse_chunks([text[a:b] for a, b in zip(edges[:-1], edges[1:])])
        assert fa.same(r, whole) is None, cut
        for k in ("n_symbols", "n_seqs", "n_ambs", "n_holes", "n_name_bytes"):
            assert sum(s[k] for s in r.summaries) == whole.summary[k], (cut, k)
    end = known()["end_text"].tobytes()
    whole = fa.parse(end)
    for c in range(len(end) + 1):
        r = fa.parse_chunks([end[:c], end[c:]])
        assert fa.same(r, whole) is None and r.summaries[-1]["status"] == fa.STATUS_END_BYTE
        assert r.summaries[1]["consumed_bytes"] == max(0, whole.summary["consumed_bytes"] - c)


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_path_equals_the_serial_loop(seed):
    rng = np.random.default_rng(100 + seed)
    alphabet = np.frombuffer(b"> \nACGTNnRY-\r\xff", dtype=np.uint8)
    p = np.array([1, 2, 4, 10, 10, 10, 10, 6, 3, 2, 2, 1, 1, 0.05 if seed % 2 else 0.0])
    text = b"xx\n" * seed + alphabet[rng.choice(len(alphabet), 5000, p=p / p.sum())].tobytes()
    a, b = fa.parse(text), fa.parse_fast(text)
    assert fa.same(a, b) is None and a.summary == b.summary
