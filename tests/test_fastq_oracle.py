"""CPU-only: the restatement of the FASTQ grammar (tests/fastq_cpu.py) against answers written out by hand (tests/golden/fastq_known.txt),
the machine as a composition of per-byte functions against the serial loop, the vectorised fast path against the serial loop, and the
round trip of well-formed records.  The GPU tests compare the library with this restatement byte for byte."""
import importlib.util
import os

import numpy as np
import pytest

import fastq_cpu as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def known():
    return np.load(os.path.join(GOLDEN, "fastq_known.npz"))


def expected_from_known(z, tag, strand_op, encoding, truncate_len):
    """the hand-written NO_OP answers of one file under an operator, an encoding and a truncation, by the definitions alone -> the arrays"""
    ri = z[tag + "_read_index"].astype(np.int64)
    syms, quals, lens = [], [], []
    for i in range(len(ri) - 1):
        s, q = z[tag + "_symbols"][ri[i]:ri[i + 1]][:truncate_len], z[tag + "_quals"][ri[i]:ri[i + 1]][:truncate_len]
        if strand_op & fc.REVERSE_OP:
            s, q = s[::-1], q[::-1]
        if strand_op & fc.COMPLEMENT_OP:
            s = np.where(s < 4, 3 - s, 4).astype(np.uint8)
        syms.append(s)
        quals.append(q)
        lens.append(len(s))
    read_index = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return cat(syms), fc.convert_qualities(cat(quals), encoding), read_index


def test_the_packed_answers_are_the_files():
    spec = importlib.util.spec_from_file_location("make_fastq_known", os.path.join(GOLDEN, "make_fastq_known.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    packed, z = mod.pack(), known()
    assert sorted(packed) == sorted(z.files)
    for k in packed:
        assert np.array_equal(packed[k], z[k]), k


def test_the_known_file_holds_what_it_is_for():
    z = known()
    text = z["known_text"].tobytes()
    ri, q = z["known_read_index"], z["known_quals"].tobytes()
    quals = [q[a:b] for a, b in zip(ri[:-1], ri[1:])]
    assert any(x.startswith(b"@") for x in quals) and b"@+@+" in quals and b"\x00" in text and b"\r" in text
    assert b"\n\n   \n" in text and not text.endswith(b"\n") and min(q) < 33 and 5 in z["known_symbols"]
    assert z["marker_summary"][0] == fc.STATUS_MARKER


@pytest.mark.parametrize("tag", ["known", "marker"])
@pytest.mark.parametrize("strand_op", [fc.NO_OP, fc.REVERSE_OP, fc.COMPLEMENT_OP, fc.REVERSE_COMPLEMENT_OP])
@pytest.mark.parametrize("encoding", [fc.PHRED, fc.PHRED33])
def test_restatement_equals_the_hand_written_answers(tag, strand_op, encoding):
    z = known()
    truncate_len = 4
    b = fc.parse(z[tag + "_text"].tobytes(), encoding, strand_op, truncate_len)
    syms, quals, read_index = expected_from_known(z, tag, strand_op, encoding, truncate_len)
    assert np.array_equal(b.read_index, read_index) and np.array_equal(b.name_index, z[tag + "_name_index"]) and np.array_equal(b.names, z[tag + "_names"])
    assert np.array_equal(fc.unpack4(b.reads4, b.read_index[-1]), syms) and np.array_equal(b.reads4, fc.pack4(syms))
    assert np.array_equal(b.quals, quals)
    status, first_bad, consumed, error_offset, error_char = (int(v) for v in z[tag + "_summary"])
    s = b.summary
    assert (s["status"], s["first_bad_record"], s["consumed_bytes"], s["error_offset"], s["error_char"]) == (status, first_bad, consumed, error_offset, error_char)
    assert s["n_records"] == len(read_index) - 1 and s["n_symbols"] == read_index[-1] and s["n_name_bytes"] == len(z[tag + "_names"])
    assert s["max_read_len"] == int(np.diff(read_index.astype(np.int64)).max()) and s["max_name_len"] == int(np.diff(z[tag + "_name_index"].astype(np.int64)).max())


def test_solexa_table_and_wrapping_arithmetic():
    q = np.arange(256, dtype=np.uint8)
    assert list(fc.convert_qualities(q, fc.SOLEXA)[:22]) == [0, 1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 10, 11]
    assert fc.convert_qualities(q, fc.SOLEXA)[255] == 245 and fc.convert_qualities(q, fc.PHRED33)[0] == 223 and fc.convert_qualities(q, fc.PHRED64)[63] == 255


def soups(rng, n, length):
    alphabet = np.frombuffer(b"@+\n AI\r\x00", dtype=np.uint8)
    return [alphabet[rng.integers(0, len(alphabet), length)].tobytes() for _ in range(n)]


def test_composition_over_random_tilings_gives_the_serial_states():
    rng = np.random.default_rng(7)
    z = known()
    texts = [z["known_text"].tobytes(), z["marker_text"].tobytes(), fc.random_records(rng, 12)] + soups(rng, 12, 200)
    texts.append(b"  \n" + fc.random_records(rng, 3) + b"x" + fc.random_records(rng, 2))
    for text in texts:
        want = fc.states_serial(text)
        for _ in range(4):
            cuts = rng.integers(1, max(len(text), 2), int(rng.integers(0, 12)))
            assert np.array_equal(fc.states_by_composition(text, cuts), want)
    # composition is associative on these functions, in stacks
    f, g, h = (fc.BYTE_FUNCTIONS[rng.integers(0, 256, 64)] for _ in range(3))
    assert np.array_equal(fc.compose(fc.compose(f, g), h), fc.compose(f, fc.compose(g, h)))


def test_the_serial_states_are_the_parser_s():
    """the record ends of states_serial (QUAL -> GAP) and its first ERR are the parser's records and marker error"""
    rng = np.random.default_rng(11)
    for text in soups(rng, 40, 120) + [fc.random_records(rng, 8) + b"?" + fc.random_records(rng, 2)]:
        st = fc.states_serial(text)
        prev = np.concatenate([[fc.GAP], st[:-1]])
        b = fc.parse(text)
        assert int(((prev == fc.QUAL) & (st == fc.GAP)).sum()) == b.n
        err = np.flatnonzero(st == fc.ERR)
        assert (len(err) > 0) == bool(b.summary["status"] & fc.STATUS_MARKER)
        if len(err):
            assert err[0] == b.summary["error_offset"] == b.summary["consumed_bytes"] and text[err[0]] == b.summary["error_char"]
        elif len(st) and st[-1] != fc.GAP:
            assert b.summary["status"] & fc.STATUS_INCOMPLETE and text[b.summary["consumed_bytes"]] == ord("@")
        else:
            assert b.summary["consumed_bytes"] == len(text)


@pytest.mark.parametrize("strand_op", [fc.NO_OP, fc.REVERSE_COMPLEMENT_OP])
def test_fast_path_equals_the_serial_loop(strand_op):
    rng = np.random.default_rng(3)
    for text, trunc in ((fc.uniform_records(rng, 50, 37, name_len=9), fc.UNLIMITED), (fc.random_records(rng, 60, multiline=0.0).replace(b"\n\n", b"\n"), 11), (b"", 5)):
        a, b = fc.parse(text, fc.PHRED33, strand_op, trunc), fc.parse_fast(text, fc.PHRED33, strand_op, trunc)
        assert a.summary == b.summary
        for k in ("reads4", "read_index", "quals", "names", "name_index"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_cap_and_chunking_rules():
    rng = np.random.default_rng(5)
    text = b"\n " + fc.random_records(rng, 6) + b"  \n"
    whole = fc.parse(text)
    assert whole.n == 6 and whole.summary["consumed_bytes"] == len(text)
    assert fc.parse(text, max_records=0).summary["consumed_bytes"] == 0
    at = 0
    for i in range(6):                                                            # one record at a time: each call stops behind its record's last byte
        one = fc.parse(text[at:], max_records=1)
        assert one.n == 1 and one.name(0) == whole.name(i) and text[at + one.summary["consumed_bytes"] - 1] == 10
        at += one.summary["consumed_bytes"]
    assert fc.parse(text[at:]).n == 0 and fc.parse(text[at:]).summary["consumed_bytes"] == len(text) - at
    for cut in range(len(text)):                                                  # every cut: first part, then its tail and the rest
        a = fc.parse(text[:cut])
        b = fc.parse(text[a.summary["consumed_bytes"]:])
        assert a.n + b.n == 6 and not a.summary["status"] & fc.STATUS_MARKER
        assert np.array_equal(np.concatenate([a.quals, b.quals]), whole.quals)


def test_leading_spaces_only_move_the_offsets():
    """what the GPU boundary sweep relies on to compute its reference once"""
    z = known()
    for text in (z["known_text"].tobytes(), z["marker_text"].tobytes(), b"", b"@a\nA\n+\nI\n"):
        base = fc.parse(text, fc.PHRED33, fc.REVERSE_OP)
        for k in (1, 15, 16, 17, 4096):
            a, b = fc.parse(b" " * k + text, fc.PHRED33, fc.REVERSE_OP), fc.shifted(base, k)
            assert a.summary == b.summary and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("reads4", "read_index", "quals", "names", "name_index"))


def test_round_trip_of_well_formed_records():
    rng = np.random.default_rng(9)
    text = fc.random_records(rng, 30, multiline=0.0)
    b = fc.parse(text)
    lines = [l for l in text.split(b"\n") if l]
    assert b.n == len(lines) // 4 and b.summary["status"] == 0
    for i in range(b.n):
        seq = bytes(b"ACGTN"[s] for s in b.symbols(i))
        assert seq == lines[4 * i + 1].upper() and bytes(b.qualities(i) + 33) == lines[4 * i + 3] and b.name(i) == lines[4 * i][1:]
