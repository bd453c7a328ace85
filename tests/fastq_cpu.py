"""The FASTQ grammar of include/nvbio_amd.h ("FASTQ input") restated on the CPU: the yardstick of the FASTQ tests.

`parse` is the reference's loop (SequenceDataFile_FASTQ_parser::nextChunk, nvbio/io/sequence/sequence_fastq.cpp:39-203) one byte at a
time, with SequenceDataEncoder::push_back's encoding (sequence_encoder.cpp:30-107,304-368) in numpy, and the departures the header lists:
qualities are reversed exactly when the symbols are, symbols beyond the kept sequence are 4 (N), an empty record is delivered, names carry
no NUL.  It takes the parameters of the device calls and returns their arrays and summary.

`byte_functions` / `compose` / `states_by_composition` restate the same machine as functions over its six states, the form the device
scans; `states_serial` is the loop they must agree with.  `parse_fast` is a vectorised path for well-formed four-line files."""
import numpy as np

PHRED, PHRED33, PHRED64, SOLEXA = 0, 1, 2, 3
NO_OP, REVERSE_OP, COMPLEMENT_OP, REVERSE_COMPLEMENT_OP = 0, 1, 2, 3
STATUS_MARKER, STATUS_INCOMPLETE, STATUS_LENGTH, STATUS_EMPTY, STATUS_CAPACITY = 1, 2, 4, 8, 16
UNLIMITED = 0xFFFFFFFF
NONE = 0xFFFFFFFF
SUMMARY_FIELDS = ("n_records", "consumed_bytes", "n_symbols", "n_name_bytes", "max_read_len", "max_name_len", "status", "error_offset",
                  "error_char", "first_bad_record")

NL, SP, AT, PLUS, NUL = 10, 32, 64, 43, 0

# nst_nt4 (sequence_encoder.cpp:30-47) as data
NT4 = np.full(256, 4, dtype=np.uint8)
for _c, _v in ((b"Aa", 0), (b"Cc", 1), (b"Gg", 2), (b"Tt", 3), (b"-", 5)):
    for _b in _c:
        NT4[_b] = _v
COMPLEMENT = np.array([3, 2, 1, 0] + [4] * 12, dtype=np.uint8)                   # bp < 4 ? 3 - bp : 4
# s_solexa_to_phred (:57-85): twenty entries, then q - 10
SOLEXA_TO_PHRED = np.array([0, 1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10] + list(range(10, 246)), dtype=np.uint8)
assert len(SOLEXA_TO_PHRED) == 256


def convert_qualities(q, encoding):
    """convert_to_phred_quality (:53-107) in uint8 arithmetic"""
    q = np.asarray(q, dtype=np.uint8)
    if encoding == PHRED:
        return q.copy()
    if encoding == PHRED33:
        return (q.astype(np.int32) - 33).astype(np.uint8)
    if encoding == PHRED64:
        return (q.astype(np.int32) - 64).astype(np.uint8)
    assert encoding == SOLEXA
    return SOLEXA_TO_PHRED[q]


def pack4(symbols):
    """4 bits per symbol, big-endian in 32-bit words: symbol i in bits 28 - 4 * (i % 8) of word i / 8"""
    s = np.asarray(symbols, dtype=np.uint32)
    padded = np.zeros((len(s) + 7) // 8 * 8, dtype=np.uint32)
    padded[:len(s)] = s
    shifts = (28 - 4 * np.arange(8)).astype(np.uint32)
    return (padded.reshape(-1, 8) << shifts).sum(axis=1).astype(np.uint32)


def unpack4(words, n):
    w = np.asarray(words, dtype=np.uint32)
    shifts = (28 - 4 * np.arange(8)).astype(np.uint32)
    return ((w[:, None] >> shifts) & 15).astype(np.uint8).reshape(-1)[:n]


class Batch:
    """what the device calls give: reads4 (uint32 words), read_index / name_index (uint32, n + 1), quals, names (uint8), summary (dict)"""

    def __init__(self, reads4, read_index, quals, names, name_index, summary):
        self.reads4, self.read_index, self.quals, self.names, self.name_index, self.summary = reads4, read_index, quals, names, name_index, summary

    @property
    def n(self):
        return self.summary["n_records"]

    def name(self, i):
        return self.names[self.name_index[i]:self.name_index[i + 1]].tobytes()

    def symbols(self, i):
        return unpack4(self.reads4, self.read_index[-1])[self.read_index[i]:self.read_index[i + 1]]

    def qualities(self, i):
        return self.quals[self.read_index[i]:self.read_index[i + 1]]


def _encode_record(seq, qual, encoding, strand_op, truncate_len):
    """push_back (:304-368): the read has the QUALITY line's length, cut to truncate_len; the strand operator works on what is left"""
    length = min(len(qual), truncate_len)
    sym = np.full(length, 4, dtype=np.uint8)                                      # departure 2: N beyond the kept sequence
    k = min(length, len(seq))
    sym[:k] = NT4[np.frombuffer(seq[:k], dtype=np.uint8)]
    q = convert_qualities(np.frombuffer(qual[:length], dtype=np.uint8), encoding)
    if strand_op & REVERSE_OP:
        sym, q = sym[::-1], q[::-1]                                               # departure 1: qualities follow the symbols
    if strand_op & COMPLEMENT_OP:
        sym = COMPLEMENT[sym]
    return sym, q


def parse(text, quality_encoding=PHRED33, strand_op=NO_OP, truncate_len=UNLIMITED, max_records=UNLIMITED):
    """the sequential machine over `text` (bytes) -> Batch"""
    text = bytes(text)
    n = len(text)
    pos = 0
    names, syms, quals, name_lens, read_lens = [], [], [], [], []
    status, error_offset, error_char, first_bad, consumed = 0, NONE, 0, NONE, 0

    def get():                                                                     # sequence_fastq.h:123-137: 0 at the end of the text
        nonlocal pos
        if pos >= n:
            return 0, False
        pos += 1
        return text[pos - 1], True

    while len(names) < max_records:                                                # :51
        consumed = pos
        while True:                                                                # :55-62
            marker, ok = get()
            if not ok or (marker != NL and marker != SP):
                break
        if not ok:                                                                 # :65: the end of the text between records
            consumed = n
            break
        if marker != AT:                                                           # :70-75
            status |= STATUS_MARKER
            error_offset, error_char, consumed = pos - 1, marker, pos - 1
            break
        start = pos - 1
        name = bytearray()
        c, ok = get()
        while ok and c != NL and c != NUL:                                         # :79-88
            name.append(c)
            c, ok = get()
        seq = bytearray()
        if ok:
            c, ok = get()
            while ok and c != PLUS and c != NUL:                                   # :103-117
                if 0x21 <= c <= 0x7E:
                    seq.append(c)
                c, ok = get()
        if ok:
            c, ok = get()
            while ok and c != NL and c != NUL:                                     # :129
                c, ok = get()
        qual = bytearray()
        if ok:
            c, ok = get()
            while ok and c != NL and c != NUL:                                     # :144-145
                qual.append(c)
                c, ok = get()
        if not ok:                                                                 # "incomplete read!"
            status |= STATUS_INCOMPLETE
            consumed = start
            break
        i = len(names)
        if len(qual) != len(seq):
            status |= STATUS_LENGTH
            first_bad = min(first_bad, i)
        if len(qual) == 0:                                                         # departure 3
            status |= STATUS_EMPTY
            first_bad = min(first_bad, i)
        s, q = _encode_record(bytes(seq), bytes(qual), quality_encoding, strand_op, truncate_len)
        names.append(bytes(name))
        syms.append(s)
        quals.append(q)
        name_lens.append(len(name))
        read_lens.append(len(s))
        consumed = pos

    read_index = np.zeros(len(names) + 1, dtype=np.uint32)
    name_index = np.zeros(len(names) + 1, dtype=np.uint32)
    read_index[1:] = np.cumsum(read_lens, dtype=np.int64)
    name_index[1:] = np.cumsum(name_lens, dtype=np.int64)
    all_syms = np.concatenate(syms) if syms else np.zeros(0, dtype=np.uint8)
    summary = dict(n_records=len(names), consumed_bytes=consumed, n_symbols=int(read_index[-1]), n_name_bytes=int(name_index[-1]),
                   max_read_len=max(read_lens or [0]), max_name_len=max(name_lens or [0]), status=status, error_offset=error_offset,
                   error_char=error_char, first_bad_record=first_bad)
    return Batch(pack4(all_syms), read_index, np.concatenate(quals) if quals else np.zeros(0, dtype=np.uint8),
                 np.frombuffer(b"".join(names), dtype=np.uint8).copy(), name_index, summary)


def shifted(batch, k):
    """the Batch of k spaces in front of a text, from the Batch of the text: leading spaces move the offsets and nothing else"""
    s = dict(batch.summary)
    s["consumed_bytes"] += k
    if s["error_offset"] != NONE:
        s["error_offset"] += k
    return Batch(batch.reads4, batch.read_index, batch.quals, batch.names, batch.name_index, s)


# ---- the machine as functions over its states ------------------------------------------------------------------------------------
GAP, NAME, SEQ, PLUS_LINE, QUAL, ERR = range(6)


def _step(state, c):
    """one byte of the loop above, as a transition"""
    if state == GAP:
        return GAP if c in (NL, SP) else NAME if c == AT else ERR
    if state == NAME:
        return SEQ if c in (NL, NUL) else NAME
    if state == SEQ:
        return PLUS_LINE if c in (PLUS, NUL) else SEQ
    if state == PLUS_LINE:
        return QUAL if c in (NL, NUL) else PLUS_LINE
    if state == QUAL:
        return GAP if c in (NL, NUL) else QUAL
    return ERR


def states_serial(text):
    """the state BEHIND every byte, from GAP"""
    out = np.zeros(len(text), dtype=np.uint8)
    s = GAP
    for i, c in enumerate(bytes(text)):
        s = _step(s, c)
        out[i] = s
    return out


# one function per byte value: row c = where each of the six states goes
BYTE_FUNCTIONS = np.array([[_step(s, c) for s in range(6)] for c in range(256)], dtype=np.uint8)
IDENTITY = np.arange(6, dtype=np.uint8)


def compose(f, g):
    """f, then g: (f then g)[s] = g[f[s]]; works on stacks of functions [..., 6]"""
    return np.take_along_axis(np.broadcast_to(g, np.broadcast_shapes(f.shape, g.shape)), np.broadcast_to(f, np.broadcast_shapes(f.shape, g.shape)).astype(np.int64), axis=-1)


def fold(functions):
    """the composition of a run of functions [k, 6], in order"""
    f = IDENTITY
    for g in functions:
        f = compose(f, g)
    return f


def states_by_composition(text, cuts):
    """the state behind every byte by the route the device takes: the text is cut into tiles at `cuts`, each tile is folded on its own,
    the tiles' functions are scanned, and each tile is walked from the state the scan gives it"""
    data = np.frombuffer(bytes(text), dtype=np.uint8)
    bounds = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(data))) + [len(data)]
    tiles = [BYTE_FUNCTIONS[data[a:b]] for a, b in zip(bounds[:-1], bounds[1:])]
    totals = [fold(t) for t in tiles]
    out = np.zeros(len(data), dtype=np.uint8)
    before = IDENTITY
    for (a, b), t, total in zip(zip(bounds[:-1], bounds[1:]), tiles, totals):
        s = before[GAP]
        f = IDENTITY
        for k in range(b - a):                                                     # inside a tile: the prefix functions applied to the entry state
            f = compose(f, t[k])
            out[a + k] = f[s]
        before = compose(before, total)
    return out


# ---- well-formed four-line files, vectorised ---------------------------------------------------------------------------------------
def parse_fast(text, quality_encoding=PHRED33, strand_op=NO_OP, truncate_len=UNLIMITED):
    """`parse` for a text of four-line records, every line ended by '\\n', no blank lines, names without NUL, sequences of 0x21..0x7E without
    '+', qualities as long as their sequences and not empty; asserts that shape"""
    data = np.frombuffer(bytes(text), dtype=np.uint8)
    nl = np.flatnonzero(data == NL)
    assert len(data) == 0 or (data[-1] == NL and len(nl) % 4 == 0)
    n = len(nl) // 4
    ends = nl.reshape(n, 4)
    starts = np.concatenate([[0], nl[:-1] + 1])[:4 * n].reshape(n, 4)
    assert np.all(data[starts[:, 0]] == AT) and np.all(data[starts[:, 2]] == PLUS) and not np.any(data == NUL)
    name_len = ends[:, 0] - starts[:, 0] - 1
    seq_len = ends[:, 1] - starts[:, 1]
    assert np.array_equal(seq_len, ends[:, 3] - starts[:, 3]) and np.all(seq_len > 0)
    length = np.minimum(seq_len, truncate_len)
    read_index = np.zeros(n + 1, dtype=np.int64)
    read_index[1:] = np.cumsum(length)
    name_index = np.zeros(n + 1, dtype=np.int64)
    name_index[1:] = np.cumsum(name_len)
    rec = np.repeat(np.arange(n), length)
    k = np.arange(read_index[-1]) - read_index[rec]
    j = length[rec] - 1 - k if strand_op & REVERSE_OP else k
    seq_bytes = data[starts[rec, 1] + j]
    assert np.all((seq_bytes >= 0x21) & (seq_bytes <= 0x7E) & (seq_bytes != PLUS))
    sym = NT4[seq_bytes]
    if strand_op & COMPLEMENT_OP:
        sym = COMPLEMENT[sym]
    quals = convert_qualities(data[starts[rec, 3] + j], quality_encoding)
    nrec = np.repeat(np.arange(n), name_len)
    names = data[starts[nrec, 0] + 1 + np.arange(name_index[-1]) - name_index[nrec]]
    summary = dict(n_records=n, consumed_bytes=len(data), n_symbols=int(read_index[-1]), n_name_bytes=int(name_index[-1]),
                   max_read_len=int(length.max()) if n else 0, max_name_len=int(name_len.max()) if n else 0, status=0, error_offset=NONE,
                   error_char=0, first_bad_record=NONE)
    return Batch(pack4(sym), read_index.astype(np.uint32), quals, names.copy(), name_index.astype(np.uint32), summary)


# ---- test files --------------------------------------------------------------------------------------------------------------------
def random_records(rng, n, min_len=1, max_len=40, multiline=0.2, name_len=(1, 12)):
    """structured random well-formed records -> bytes; with probability `multiline` a sequence is broken over lines"""
    out = bytearray()
    for i in range(n):
        length = int(rng.integers(min_len, max_len + 1))
        name = bytes(rng.choice(np.frombuffer(b"abcXYZ019_/:.", dtype=np.uint8), int(rng.integers(name_len[0], name_len[1] + 1))).astype(np.uint8))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTNacgt", dtype=np.uint8), length).astype(np.uint8))
        qual = bytes(rng.integers(33, 74, length).astype(np.uint8))
        if rng.random() < multiline and length > 2:
            cut = sorted(set(int(c) for c in rng.integers(1, length, 2)))
            seq = b"\n".join([seq[:cut[0]]] + [seq[a:b] for a, b in zip(cut, cut[1:] + [length])])
        out += b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"
        if rng.random() < 0.1:
            out += b"\n"
    return bytes(out)


def uniform_records(rng, n, read_len, name_len=20):
    """n four-line records of read_len symbols with name_len-byte names -> bytes, built without a Python loop"""
    line = name_len + 2 + read_len + 1 + 2 + read_len + 1
    a = np.zeros((n, line), dtype=np.uint8)
    a[:, 0] = AT
    digits = np.arange(n)[:, None] // 10 ** np.arange(name_len - 2, -1, -1)[None, :] % 10 if name_len > 1 else np.zeros((n, 0), dtype=np.int64)
    a[:, 1] = ord("r")
    a[:, 2:name_len + 1] = 48 + digits
    a[:, name_len + 1] = NL
    s0 = name_len + 2
    a[:, s0:s0 + read_len] = np.frombuffer(b"ACGTN", dtype=np.uint8)[np.minimum(rng.integers(0, 41, (n, read_len)) // 10, 4)]
    a[:, s0 + read_len] = NL
    a[:, s0 + read_len + 1] = PLUS
    a[:, s0 + read_len + 2] = NL
    q0 = s0 + read_len + 3
    a[:, q0:q0 + read_len] = rng.integers(33, 74, (n, read_len))
    a[:, q0 + read_len] = NL
    return a.tobytes()
