"""A plain restatement of the FASTA grammar of include/nvbio_amd.h ("FASTA input"): the reference's FASTA_inc_reader::read feeding
nvBWT's Writer (nvbio/fasta/fasta_inl.h:64-122, nvBWT/nvBWT.cu:102-195) with the departures the header lists.  `Parser` is the serial
byte loop with the chunk carry; `parse_fast` is a vectorised numpy path for large inputs; `byte_fn` / `compose` restate the machine as
functions over its five states.  tests/test_fasta_oracle.py pins all of this to hand-written answers; the GPU tests compare the
library with it byte for byte.  No device code is used here."""
import numpy as np

PRE, ID, REST, BODY, END = range(5)
NO_SYMBOL = 0x100
STATUS_INCOMPLETE, STATUS_END_BYTE, STATUS_OVERFLOW_32, STATUS_CAPACITY = 1, 2, 4, 8
SUMMARY_FIELDS = ("n_symbols", "n_seqs", "n_ambs", "n_holes", "n_name_bytes", "consumed_bytes", "machine", "status")

LCG_A, LCG_C, LCG_MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1

CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _i


# ---- drand48 ----------------------------------------------------------------------------------------------------------------------
def lcg_seed(seed):
    return ((seed << 16) | 0x330E) & LCG_MASK


def lcg_step(x):
    return (LCG_A * x + LCG_C) & LCG_MASK


def lcg_jump(x, steps):
    """x after `steps` steps: the 2^j-step maps (a, c) applied for every set bit of steps"""
    a, c = LCG_A, LCG_C
    while steps:
        if steps & 1:
            x = (a * x + c) & LCG_MASK
        c = (a * c + c) & LCG_MASK
        a = (a * a) & LCG_MASK
        steps >>= 1
    return x


def draw(seed, k):
    """the k-th draw, k from 0: uint8( drand48() * 4 ) & 3 after srand48( seed )"""
    return lcg_jump(lcg_seed(seed), k + 1) >> 46


def draws(seed, first, count):
    """draws first .. first + count - 1 as a uint8 array, by doubling: X[m : 2m] = the m-step map of X[0 : m]"""
    if count == 0:
        return np.zeros(0, np.uint8)
    x = np.zeros(count, dtype=np.uint64)
    x[0] = lcg_jump(lcg_seed(seed), first + 1)
    m, a, c = 1, LCG_A, LCG_C
    while m < count:
        k = min(m, count - m)
        x[m:m + k] = (np.uint64(a) * x[:k] + np.uint64(c)) & np.uint64(LCG_MASK)           # uint64 wraps mod 2^64: the low 48 bits are exact
        c = (a * c + c) & LCG_MASK
        a = (a * a) & LCG_MASK
        m += k
    return (x >> np.uint64(46)).astype(np.uint8)


# ---- the machine as functions -------------------------------------------------------------------------------------------------------
def next_state(s, c):
    if s == PRE:
        return ID if c == 0x3E else END if c == 0xFF else PRE
    if s == ID:
        return REST if c == 0x20 else BODY if c == 0x0A else ID
    if s == REST:
        return BODY if c == 0x0A else REST
    if s == BODY:
        return ID if c == 0x3E else END if c == 0xFF else BODY
    return END


def byte_fn(c):
    return tuple(next_state(s, c) for s in range(5))


IDENTITY = tuple(range(5))


def compose(f, g):
    """f, then g"""
    return tuple(g[f[s]] for s in range(5))


def pack2(symbols):
    """codes 0..3 -> big-endian 2-bit words: symbol i in bits 30 - 2 * (i % 16) of word i / 16"""
    n = len(symbols)
    s = np.zeros((n + 15) // 16 * 16, dtype=np.uint32)
    s[:n] = symbols
    return (s.reshape(-1, 16) << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def unpack2(words, n):
    w = np.asarray(words, dtype=np.uint32)
    return ((w[:, None] >> (30 - 2 * np.arange(16, dtype=np.uint32))) & 3).astype(np.uint8).reshape(-1)[:n]


# ---- the serial loop ----------------------------------------------------------------------------------------------------------------
class Parser:
    """The byte loop with the Writer's semantics.  feed() takes a chunk cut anywhere and returns that chunk's summary (the fields of
    nvbio_fasta_summary); finish() closes the tables.  The attributes are the totals so far."""

    def __init__(self, seed=11):
        self.seed, self.machine, self.x = seed, PRE, lcg_seed(seed)
        self.symbols, self.raw = [], []                   # the stored codes and the bytes they came from
        self.seq_offset, self.name_index, self.names = [], [], bytearray()
        self.hole_offset, self.hole_len, self.hole_amb, self.hole_rank = [], [], [], []
        self.n_ambs, self.last_symbol, self.freq = 0, NO_SYMBOL, [0, 0, 0, 0]
        self.status = 0

    def state(self):
        """the fields of nvbio_fasta_state that the calls set (max_name_len is finish's)"""
        return dict(machine=self.machine, n_symbols=len(self.symbols), n_seqs=len(self.seq_offset), n_ambs=self.n_ambs, n_holes=len(self.hole_offset),
                    n_name_bytes=len(self.names), last_symbol=self.last_symbol, seed=self.seed, freq=list(self.freq))

    def feed(self, chunk):
        before = self.state()
        consumed = len(chunk)
        for p, c in enumerate(bytes(chunk)):
            s = self.machine
            if s == END:
                consumed = min(consumed, p)
                break
            if s in (PRE, BODY):
                if c == 0xFF:
                    consumed = p
                elif c == 0x3E:                                            # begin_read: m_lasts is forgotten (departure d: no byte equals it)
                    self.seq_offset.append(len(self.symbols))
                    self.name_index.append(len(self.names))
                    self.last_symbol = NO_SYMBOL
                elif s == BODY and c not in (0x0A, 0x20):
                    self._symbol(c)
            elif s == ID and c not in (0x20, 0x0A):
                self.names.append(c)
            self.machine = next_state(s, c)
        status = 0
        if self.machine in (ID, REST):
            status |= STATUS_INCOMPLETE
        if self.machine == END:
            status |= STATUS_END_BYTE
        self.status = status
        now = self.state()
        out = {k: now[k] - before[k] for k in ("n_symbols", "n_seqs", "n_ambs", "n_holes", "n_name_bytes")}
        out.update(consumed_bytes=consumed, machine=self.machine, status=status)
        return out

    def _symbol(self, c):
        code = int(CODE[c])
        if code >= 4:
            self.x = lcg_step(self.x)
            code = self.x >> 46
            if self.last_symbol == c:
                self.hole_len[-1] += 1
            else:
                self.hole_offset.append(len(self.symbols))
                self.hole_len.append(1)
                self.hole_amb.append(c)
                self.hole_rank.append(self.n_ambs)
            self.n_ambs += 1
        self.symbols.append(code)
        self.raw.append(c)
        self.freq[code] += 1
        self.last_symbol = c

    def finish(self):
        return Reference(np.array(self.symbols, dtype=np.uint8), np.array(self.seq_offset + [len(self.symbols)], dtype=np.uint32),
                         np.frombuffer(bytes(self.names), dtype=np.uint8), np.array(self.name_index + [len(self.names)], dtype=np.uint32),
                         np.array(self.hole_offset, dtype=np.uint32), np.array(self.hole_len, dtype=np.uint32), np.array(self.hole_amb, dtype=np.uint8),
                         np.array(self.hole_rank, dtype=np.uint32), self.seed, self.status, self.machine)


class Reference:
    """what a parsed reference is: symbols (the stored codes), text2 (their packed words), seq_offset and name_index (n + 1 each), names
    (bytes), the holes (offset, len, amb, rank = the ambiguous symbols before the hole), seq_n_ambs, freq, status"""

    def __init__(self, symbols, seq_offset, names, name_index, hole_offset, hole_len, hole_amb, hole_rank, seed, status, machine):
        self.symbols, self.seq_offset, self.names, self.name_index = symbols, seq_offset, names, name_index
        self.hole_offset, self.hole_len, self.hole_amb, self.hole_rank = hole_offset, hole_len, hole_amb, hole_rank
        self.seed, self.status, self.machine = seed, status, machine
        self.text2 = pack2(symbols)
        self.length, self.n_seqs, self.n_holes = len(symbols), len(seq_offset) - 1, len(hole_offset)
        self.n_ambs = int(hole_len.sum())
        self.freq = np.bincount(symbols, minlength=4).astype(np.uint32)
        lo = np.searchsorted(hole_offset, seq_offset, side="left")
        self.seq_n_ambs = (lo[1:] - lo[:-1]).astype(np.uint32)
        self.max_name_len = int((name_index[1:] - name_index[:-1]).max()) if self.n_seqs else 0

    def name_list(self):
        b = self.names.tobytes()
        return [b[self.name_index[i]:self.name_index[i + 1]] for i in range(self.n_seqs)]

    def files(self):
        """the bytes of .pac, .ann and .amb as save_bpac and save_bns write them (nvBWT.cu:243-287, bnt.cpp:28-73): gi 0, anno "null"; a name
        is printed up to its first NUL (c_str), a hole's byte with %c"""
        n = self.length
        s = np.zeros((n + 3) // 4 * 4, dtype=np.uint8)
        s[:n] = self.symbols
        q = s.reshape(-1, 4)
        pac = ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8).tobytes()
        pac += (b"\0" if n % 4 == 0 else b"") + bytes([n % 4])
        ann = b"%d %d %d\n" % (n, self.n_seqs, self.seed)
        for i, name in enumerate(self.name_list()):
            ann += b"0 " + name.split(b"\0")[0] + b" null\n"
            ann += b"%d %d %d\n" % (self.seq_offset[i], self.seq_offset[i + 1] - self.seq_offset[i], self.seq_n_ambs[i])
        amb = b"%d %d %d\n" % (n, self.n_seqs, self.n_holes)
        for o, l, a in zip(self.hole_offset, self.hole_len, self.hole_amb):
            amb += b"%d %d " % (o, l) + bytes([a]) + b"\n"
        return dict(pac=pac, ann=ann, amb=amb)


def parse(text, seed=11):
    p = Parser(seed)
    p.summary = p.feed(text)
    r = p.finish()
    r.summary = p.summary
    return r


def parse_chunks(chunks, seed=11):
    p = Parser(seed)
    summaries = [p.feed(c) for c in chunks]
    r = p.finish()
    r.summaries = summaries
    return r


# ---- the vectorised path: a whole text from PRE on ------------------------------------------------------------------------------------
def parse_fast(text, seed=11):
    """parse() for large inputs: only the header lines are walked one by one"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(t)
    gt, nl, sp, ff = (np.flatnonzero(t == c) for c in (0x3E, 0x0A, 0x20, 0xFF))
    first_at = lambda idx, p: int(idx[np.searchsorted(idx, p)]) if np.searchsorted(idx, p) < len(idx) else n
    pos, machine, end = 0, PRE, n
    starts, names, bodies = [], [], []                        # each sequence's body is t[bodies[i][0] : bodies[i][1]]
    while True:
        g, f = first_at(gt, pos), first_at(ff, pos)
        if f < g:
            if starts:
                bodies.append((pos, f))
            machine, end = END, f
            break
        if starts:
            bodies.append((pos, g))
        if g == n:
            machine = BODY if starts else PRE
            break
        line_end = first_at(nl, g + 1)
        name_end = min(first_at(sp, g + 1), line_end)
        starts.append(g)
        names.append(t[g + 1:name_end].tobytes())
        if line_end == n:
            machine = ID if name_end == n else REST
            bodies.append((n, n))
            break
        pos = line_end + 1
    raws, seq_of = [], []
    for i, (a, b) in enumerate(bodies):
        seg = t[a:b]
        seg = seg[(seg != 0x0A) & (seg != 0x20)]
        raws.append(seg)
        seq_of.append(np.full(len(seg), i, dtype=np.int64))
    raw = np.concatenate(raws) if raws else np.zeros(0, np.uint8)
    seq_of = np.concatenate(seq_of) if seq_of else np.zeros(0, np.int64)
    lens = np.array([len(r) for r in raws], dtype=np.int64)
    seq_offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    code = CODE[raw]
    amb = code >= 4
    first = np.ones(len(raw), dtype=bool)
    first[1:] = seq_of[1:] != seq_of[:-1]
    differs = np.ones(len(raw), dtype=bool)
    differs[1:] = raw[1:] != raw[:-1]
    hole = amb & (first | differs)
    symbols = code.copy()
    symbols[amb] = draws(seed, 0, int(amb.sum()))
    rank = np.cumsum(amb) - amb
    hole_offset = np.flatnonzero(hole).astype(np.uint32)
    hole_rank = rank[hole].astype(np.uint32)
    hole_len = np.diff(np.concatenate([hole_rank, [amb.sum()]])).astype(np.uint32)
    name_index = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint32)
    status = (STATUS_INCOMPLETE if machine in (ID, REST) else 0) | (STATUS_END_BYTE if machine == END else 0)
    r = Reference(symbols, seq_offset, np.frombuffer(b"".join(names), dtype=np.uint8), name_index, hole_offset, hole_len, raw[hole], hole_rank, seed, status,
                  machine)
    r.summary = dict(n_symbols=len(raw), n_seqs=len(starts), n_ambs=int(amb.sum()), n_holes=len(hole_offset), n_name_bytes=int(name_index[-1]),
                     consumed_bytes=end, machine=machine, status=status)
    return r


def same(a, b):
    """every table of two References, and what differs"""
    for k in ("symbols", "text2", "seq_offset", "names", "name_index", "hole_offset", "hole_len", "hole_amb", "hole_rank", "seq_n_ambs", "freq"):
        if not np.array_equal(getattr(a, k), getattr(b, k)):
            return k
    for k in ("status", "machine", "length", "n_ambs", "max_name_len"):
        if getattr(a, k) != getattr(b, k):
            return k
    return None
