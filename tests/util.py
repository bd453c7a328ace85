"""shared helpers for the parity tests"""
import numpy as np


def make_queries(rng, text, Q, min_len=1, max_len=32, hit_every=2, n_count=0):
    """concatenated query set: every `hit_every`-th query is a substring of text, others random"""
    n = len(text)
    lens = rng.integers(min_len, max_len + 1, Q)
    offs = np.zeros(Q + 1, dtype=np.uint32)
    offs[1:] = np.cumsum(lens)
    syms = rng.integers(0, 4, int(offs[-1]), dtype=np.uint8)
    for q in range(0, Q, hit_every):
        if lens[q] <= n:
            p = int(rng.integers(0, n - lens[q] + 1))
            syms[offs[q]:offs[q + 1]] = text[p:p + lens[q]]
    if n_count:
        syms[rng.integers(0, len(syms), n_count)] = 4
    return syms, offs


def mutate_reads(rng, text, starts, M, sub=0.02, indel=0.1):
    """reads of length M drawn at `starts`, with substitutions and an occasional 1-3 bp indel"""
    reads = np.zeros((len(starts), M), dtype=np.uint8)
    for k, s in enumerate(starts):
        r = text[s:s + M + 8].copy()
        if rng.random() < indel:
            p = int(rng.integers(5, M - 5)); g = int(rng.integers(1, 4))
            if rng.random() < 0.5:
                r = np.concatenate([r[:p], r[p + g:]])
            else:
                r = np.concatenate([r[:p], rng.integers(0, 4, g, dtype=np.uint8), r[p:]])
        r = r[:M]
        m = rng.random(M) < sub
        r[m] = rng.integers(0, 4, int(m.sum()))
        reads[k] = r
    return reads


# ---------------------------------------------------------------------------------------------
# the reference's results, recorded: tests/test_oracle_vs_reference.py runs against the reference's own host code
# (oracle/_ref) where it is built, and against what that code returned for the same calls everywhere else
# ---------------------------------------------------------------------------------------------
REF_RECORDING = "ref_fuzz_golden.npz"
_PASSTHROUGH = ("adopt_index", "destroy", "num_threads", "set_num_threads")


def _flatten(x):
    """a result of the reference's bindings -> (structure code, leaves): tuples nest, 'a' an array, 'i' an integer"""
    if isinstance(x, tuple):
        codes, leaves = [], []
        for e in x:
            c, l = _flatten(e)
            codes.append(c); leaves += l
        return "(" + ",".join(codes) + ")", leaves
    if isinstance(x, np.ndarray):
        return "a", [x]
    if isinstance(x, (int, np.integer)):
        return "i", [np.asarray(int(x), dtype=np.int64)]
    raise TypeError("cannot record a %s" % type(x).__name__)


def _unflatten(code, leaves):
    pos = [0]
    it = iter(leaves)

    def parse():
        c = code[pos[0]]
        pos[0] += 1
        if c == "a":
            return next(it)
        if c == "i":
            return int(next(it))
        out = []                                                     # c == "("
        while code[pos[0]] != ")":
            out.append(parse())
            if code[pos[0]] == ",":
                pos[0] += 1
        pos[0] += 1
        return tuple(out)
    return parse()


def _args_crc(args, kwargs):
    """crc32 of a call's inputs (an index handle counts by name only): a replay refuses calls that are not the recorded ones"""
    import zlib
    crc = 0
    for a in list(args) + [kwargs[k] for k in sorted(kwargs)]:
        if isinstance(a, np.ndarray):
            b = np.ascontiguousarray(a).tobytes() + str(a.dtype).encode()
        elif hasattr(a, "as_array"):                                 # oracle.Scheme
            b = a.as_array().tobytes()
        elif hasattr(a, "bwt_occ"):                                  # oracle.HostIndex
            b = b"index"
        elif isinstance(a, (int, np.integer, np.bool_)):
            b = str(int(a)).encode()
        else:
            b = repr(a).encode()
        crc = zlib.crc32(b, crc)
    return crc


class RecordingReference:
    """the live reference, every result logged per method in call order (tests/golden/make_golden.py)"""

    def __init__(self, ref):
        self._ref = ref
        self.log = {}

    def __getattr__(self, name):
        fn = getattr(self._ref, name)
        if name in _PASSTHROUGH:
            return fn

        def call(*args, **kwargs):
            out = fn(*args, **kwargs)
            rec = (out.n, out.primary, out.L2, out.ssa, out.sa) if name == "build_index" else out
            self.log.setdefault(name, []).append((_args_crc(args, kwargs),) + _flatten(rec))
            return out
        return call


def save_recordings(path, logs):
    """{test name: RecordingReference.log} -> one npz: per (test, method) the structure code, the inputs' crc32 per call and every
    leaf position stacked over the calls (integers as one array; arrays concatenated, with their shapes)"""
    out = {}
    for test, log in logs.items():
        for method, calls in log.items():
            key = "%s__%s__" % (test, method)
            codes = {c[1] for c in calls}
            assert len(codes) == 1, (test, method, codes)
            out[key + "code"] = np.array(codes.pop())
            out[key + "crc"] = np.array([c[0] for c in calls], dtype=np.uint32)
            for j in range(len(calls[0][2])):
                leaf = [c[2][j] for c in calls]
                if leaf[0].ndim == 0:
                    out[key + str(j)] = np.stack(leaf)
                else:
                    out[key + str(j)] = np.concatenate([a.ravel() for a in leaf])
                    out[key + str(j) + "_shape"] = np.array([a.shape for a in leaf], dtype=np.int64)
    np.savez_compressed(path, **out)


class ReplayedReference:
    """the reference's recorded results for one test, handed back in the order the test makes its calls"""

    def __init__(self, recording, test):
        self._z, self._test, self._next, self._cache = recording, test, {}, {}

    def adopt_index(self, hidx):
        return hidx

    def destroy(self, idx):
        pass

    def _method(self, name):
        if name not in self._cache:
            key = "%s__%s__" % (self._test, name)
            if key + "code" not in self._z:
                raise AttributeError("no recorded results of %s in %s (tests/golden/make_golden.py writes them)" % (name, self._test))
            code = str(self._z[key + "code"])
            crc = self._z[key + "crc"]
            leaves = []
            j = 0
            while key + str(j) in self._z:
                data = self._z[key + str(j)]
                if key + str(j) + "_shape" in self._z:
                    shapes = self._z[key + str(j) + "_shape"]
                    ends = np.cumsum([int(np.prod(s)) for s in shapes])
                    leaves.append((data, shapes, ends - [int(np.prod(s)) for s in shapes]))
                else:
                    leaves.append((data, None, None))
                j += 1
            self._cache[name] = (code, crc, leaves)
        return self._cache[name]

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        code, crc, leaves = self._method(name)

        def call(*args, **kwargs):
            i = self._next.get(name, 0)
            assert i < len(crc), "%s: call %d of %s was not recorded" % (self._test, i, name)
            assert _args_crc(args, kwargs) == crc[i], "%s: call %d of %s has other inputs than the recorded one" % (self._test, i, name)
            self._next[name] = i + 1
            vals = []
            for data, shapes, begins in leaves:
                if shapes is None:
                    vals.append(data[i])
                else:
                    b = int(begins[i])
                    vals.append(data[b:b + int(np.prod(shapes[i]))].reshape(tuple(shapes[i])).copy())
            out = _unflatten(code, vals)
            if name == "build_index":
                import oracle
                n, primary, L2, ssa, sa = out
                return oracle.HostIndex(n, primary, L2, np.zeros(0, dtype=np.uint32), ssa, sa=sa)
            return out
        return call

    def check_consumed(self):
        """every recorded call was made"""
        head = self._test + "__"
        for key in self._z.files:
            if key.startswith(head) and key.endswith("__code"):
                name = key[len(head):-len("__code")]
                made, recorded = self._next.get(name, 0), len(self._z[head + name + "__crc"])
                assert made == recorded, "%s: %d of %d recorded calls of %s made" % (self._test, made, recorded, name)


# ---------------------------------------------------------------------------------------------
# inputs for the banded DP at its numeric limits (tests/test_gpu_band31_range.py, tests/golden/make_golden.py: band31_range,
# tests/test_oracle_vs_reference.py::test_gotoh_long_fuzz)
# ---------------------------------------------------------------------------------------------
# the kinds in the order jobs take them: neighbours always differ (the two alignments of a packed lane are jobs 2p and 2p + 1), also
# round the end of the cycle; 6 of 17 are the extreme ones (all-mismatch, perfect), 5 of 17 ordinary mutated reads
RANGE_KINDS = ("allmm", "mut", "perfect", "gap", "mut", "allmm", "shift", "mutn", "perfect", "gap", "mut", "random", "allmm", "mut",
               "clip", "gap", "mut")


def _substitute(rng, r, k):
    if k and len(r):
        pos = rng.choice(len(r), min(k, len(r)), replace=False)
        r[pos] = (r[pos] + 1 + rng.integers(0, 3, len(pos))) % 4
    return r


def _mutated(rng, txt, M, W):
    """a read from somewhere inside the band with 0-5 substitutions and (M > 12) an indel of 1-3 symbols"""
    d0 = int(rng.integers(3, W - 3)) if W >= 7 else int(rng.integers(0, W))
    src = txt[d0:]
    if M > 12:
        p = int(rng.integers(1, M - 4)); g = int(rng.integers(1, 4))
        src = txt[min(d0, W - g):]                                   # (a deletion leaves M symbols of the window)
        r = (np.concatenate([src[:p], src[p + g:]]) if rng.random() < 0.5 else
             np.concatenate([src[:p], rng.integers(0, 4, g, dtype=np.uint8), src[p:]]))[:M]
    else:
        r = src[:M]
    return _substitute(rng, r.copy(), int(rng.integers(0, 6)))


def range_job(rng, kind, M, band=31, variant=0, allow_n=True):
    """one (pattern as aligned, text window) pair of a kind of RANGE_KINDS for a pattern of M symbols: the window has M + band symbols
    (BestScoreStream's) unless the kind clips it; `variant` walks through the kind's sub-cases"""
    W = band; c = W // 2; N = M + W
    txt = rng.integers(0, 4, N, dtype=np.uint8)
    if kind == "gap" and M < 4:
        kind = "shift"
    if kind == "allmm":                                              # one letter against another: every cell of the band mismatches
        a = int(rng.integers(0, 4))
        return np.full(M, a, dtype=np.uint8), np.full(N, (a + 1 + int(rng.integers(0, 3))) % 4, dtype=np.uint8)
    if kind == "perfect":                                            # on the centre diagonal
        return txt[c:c + M].copy(), txt
    if kind == "shift":                                              # window begin off by +-band/2: the best diagonal is the band's first / last
        d = 0 if variant % 2 == 0 else W - 1
        return txt[d:d + M].copy(), txt
    if kind == "gap":                                                # one gap of 1, band/2, band-1 symbols at the start, middle, end; both directions
        g = (1, max(c, 1), W - 1)[variant % 3]
        if M < g + 8:
            g = 1
        p = (min(2, M - 2), M // 2, M - 2)[(variant // 3) % 3]
        if (variant // 9) % 2 == 0:                                  # the read lacks g text symbols: the diagonal moves up by g
            d0 = int(rng.integers(0, W - g))
            return np.concatenate([txt[d0:d0 + p], txt[d0 + p + g:d0 + g + M]]), txt
        d0 = int(rng.integers(g, W))                                 # g symbols more in the read: the diagonal moves down by g
        p = min(p, M - g - 2)
        return np.concatenate([txt[d0:d0 + p], rng.integers(0, 4, g, dtype=np.uint8), txt[d0 + p:d0 + M - g]]), txt
    if kind == "random":
        return rng.integers(0, 4, M, dtype=np.uint8), txt
    r = _mutated(rng, txt, M, W)
    if kind == "mutn":
        k = int(rng.integers(1, 4))
        if allow_n:
            r[rng.integers(0, M, k)] = 4
        else:
            _substitute(rng, r, k)
    if kind == "clip":                                               # the window ends early: N < M + band - 1, every third N < M
        n = M - int(rng.integers(1, 4)) if variant % 3 == 0 else M + W - int(rng.integers(2, max(W - 1, 3)))
        txt = txt[:max(n, W - 1, 1)]                                 # (below band - 1 symbols the reference's result is undefined)
    return r, txt


def range_jobs(seed, lens, band=31, first=0, allow_n=True, kinds=None):
    """jobs of the given pattern lengths, job j of kind RANGE_KINDS[(first + j) % 17] (or kinds[j]) -> (patterns, texts, kind names)"""
    rng = np.random.default_rng(seed)
    pats, txts, names = [], [], []
    seen = {}
    for j, M in enumerate(lens):
        kind = kinds[j] if kinds is not None else RANGE_KINDS[(first + j) % len(RANGE_KINDS)]
        v = seen.get(kind, 0); seen[kind] = v + 1
        p, t = range_job(rng, kind, int(M), band, v + first, allow_n)
        assert len(p) == M and p.dtype == np.uint8 and t.dtype == np.uint8
        pats.append(p); txts.append(t); names.append(kind)
    return pats, txts, np.array(names)


def range_layout(pats, txts, quals=None, flags=None):
    """lay jobs out the way nvBowtie holds them: the windows one after another on one text (the first begins at the text's first symbol, the
    last ends at its last), the reads stored reversed and / or complemented as each job's flags say (qualities mirrored with them)
    -> dict(reads, roffs, quals, text, wb, we, flags), symbols one per byte"""
    n = len(pats)
    flags = np.zeros(n, dtype=np.uint8) if flags is None else np.asarray(flags, dtype=np.uint8)
    stored, sq = [], []
    for j in range(n):
        r = pats[j]
        q = quals[j] if quals is not None else None
        if flags[j] & 2:
            r = np.where(r < 4, 3 - r, r).astype(np.uint8)
        if flags[j] & 1:
            r = r[::-1]; q = q[::-1] if q is not None else None
        stored.append(r); sq.append(q)
    roffs = np.zeros(n + 1, dtype=np.uint32); roffs[1:] = np.cumsum([len(p) for p in pats])
    toffs = np.zeros(n + 1, dtype=np.uint32); toffs[1:] = np.cumsum([len(t) for t in txts])
    return dict(reads=np.concatenate(stored), roffs=roffs, quals=np.concatenate(sq) if quals is not None else None,
                text=np.concatenate(txts), wb=toffs[:-1].copy(), we=toffs[1:].copy(), flags=flags)


def flat_scheme(match, s):
    """every penalty the same: the schemes under which a score reaches (rows + band) * step"""
    return (match, s, s, -s, -s, -s, -s)


def scheme_step(sv):
    """the largest single penalty of a scheme"""
    return max(sv[1], sv[2], -sv[3], -sv[4], -sv[5], -sv[6])


# alignment types as the C-ABI numbers them
_GLOBAL, _LOCAL, _SEMI_GLOBAL = 0, 1, 2

# the edges of the three band-31 routes: (name, route whose limit it is, type, scheme, base qualities?).  The pattern lengths on either side
# are not listed: band31_last_admitted() computes them from the admission rules
RANGE_EDGES = (
    # binary16 lanes: SEMI_GLOBAL, match 0, (M + 32) * step <= 2040
    ("f16_flat8", "f16", _SEMI_GLOBAL, flat_scheme(0, 8), False),
    ("f16_flat10", "f16", _SEMI_GLOBAL, flat_scheme(0, 10), False),
    ("f16_flat1", "f16", _SEMI_GLOBAL, flat_scheme(0, 1), False),
    ("f16_flat60", "f16", _SEMI_GLOBAL, flat_scheme(0, 60), False),
    ("f16_ramp8", "f16", _SEMI_GLOBAL, (0, 2, 8, -8, -3, -8, -3), True),          # mm_max == step, qualities
    ("f16_asym8", "f16", _SEMI_GLOBAL, (0, 5, 5, -8, -2, -6, -3), False),         # asymmetric gap terms
    # int16 lanes: (M + 32) * step <= 8000
    ("i16_sg_flat8", "i16", _SEMI_GLOBAL, flat_scheme(0, 8), False),
    ("i16_sg_match3_flat8", "i16", _SEMI_GLOBAL, flat_scheme(3, 8), False),
    ("i16_g_flat8", "i16", _GLOBAL, flat_scheme(0, 8), False),
    ("i16_g_match8_flat8", "i16", _GLOBAL, flat_scheme(8, 8), False),
    ("i16_sg_flat40", "i16", _SEMI_GLOBAL, flat_scheme(0, 40), False),
    ("i16_g_match40_flat40", "i16", _GLOBAL, flat_scheme(40, 40), False),
    ("i16_sg_flat1", "i16", _SEMI_GLOBAL, flat_scheme(0, 1), False),
    ("i16_g_flat1", "i16", _GLOBAL, flat_scheme(0, 1), False),
    ("i16_g_match1_flat1", "i16", _GLOBAL, flat_scheme(1, 1), False),
    ("i16_sg_flat242", "i16", _SEMI_GLOBAL, flat_scheme(0, 242), False),          # M = 1: the other side is step 243
    ("i16_g_flat242", "i16", _GLOBAL, flat_scheme(0, 242), False),
    ("i16_sg_ramp8", "i16", _SEMI_GLOBAL, (0, 3, 8, -8, -3, -8, -3), True),
    ("i16_g_asym8", "i16", _GLOBAL, (2, 5, 5, -8, -2, -6, -3), False),
    # int16 lanes, LOCAL: match * M <= 1000, every penalty <= 4096
    ("i16_local_match2", "i16", _LOCAL, (2, 6, 6, -8, -3, -8, -3), False),
    ("i16_local_match1", "i16", _LOCAL, (1, 6, 6, -8, -3, -8, -3), False),
    ("i16_local_match3", "i16", _LOCAL, (3, 6, 6, -8, -8, -8, -8), False),
    ("i16_local_match5_ramp", "i16", _LOCAL, (5, 2, 6, -5, -3, -7, -2), True),
    ("i16_local_mm4096", "i16", _LOCAL, (2, 4096, 4096, -8, -3, -8, -3), False),  # the other side is a penalty of 4097
    ("i16_local_open4096", "i16", _LOCAL, (2, 6, 6, -4096, -3, -8, -3), False),
    # int32: LOCAL scores past 32,767 (perfect reads of 5,000 symbols score 45,000)
    ("i32_local_match9", "i32", _LOCAL, (9, 2, 60, -8, -3, -8, -3), False),
)


def band31_route(typ, sv, max_read_len):
    """which arithmetic nvbio_banded_gotoh_score runs band 31 in for 4- or 2-bit reads on a 2-bit text under default flags: 'f16', 'i16'
    or 'i32' -- the host's rules (packed_ok() and the binary16 condition of launch_pk_kernel(), csrc/band31_packed.hip) restated"""
    match, mm_min, mm_max, pat_go, pat_ge, txt_go, txt_ge = sv
    M, lim, step = int(max_read_len), 4096, scheme_step(sv)
    packed = M > 0 and match >= 0 and 0 <= mm_min <= lim and 0 <= mm_max <= lim and -lim <= pat_go <= 0 and -lim <= pat_ge <= 0
    if packed and typ == _LOCAL:
        packed = match * M <= 1000                                   # the sink key (score << 5 | column) fits an int16
    elif packed:
        packed = -lim <= txt_go <= 0 and -lim <= txt_ge <= 0 and (M + 32) * max(step, match) <= 8000
    if not packed:
        return "i32"
    if typ == _SEMI_GLOBAL and match == 0 and (M + 32) * step <= 2040 and mm_max <= 400:
        return "f16"
    return "i16"


def band31_last_admitted(route, typ, sv):
    """the largest max_read_len the rules admit to `route` under this scheme (None for 'i32': nothing is refused there)"""
    if route == "f16":
        return 2040 // scheme_step(sv) - 32
    if route == "i16":
        return 1000 // sv[0] if typ == _LOCAL else 8000 // max(scheme_step(sv), sv[0]) - 32
    return None


def range_edge_sides(edge):
    """an edge of RANGE_EDGES -> ((scheme, max_read_len, route) last admitted, (scheme, max_read_len, route) first refused): the next
    length, or where the length cannot grow (a penalty at its own limit; M = 1 under step 242) the next penalty"""
    name, route, typ, sv, _ = edge
    if route == "i32":
        return ((sv, 5000, "i32"),)
    M = band31_last_admitted(route, typ, sv)
    if name.endswith("4096") or name.endswith("flat242"):
        over = tuple(v + (1 if v > 0 else -1) if abs(v) == scheme_step(sv) else v for v in sv)
        sides = ((sv, M, route), (over, M, band31_route(typ, over, M)))
    else:
        sides = ((sv, M, route), (sv, M + 1, band31_route(typ, sv, M + 1)))
    assert band31_route(typ, sides[0][0], sides[0][1]) == route and sides[1][2] != route, name
    return sides


# ---------------------------------------------------------------------------------------------
# inputs for the full-matrix DP at the limits of its routes (tests/test_gpu_full_range.py, tests/golden/make_golden.py: full_range,
# tests/test_oracle_vs_reference.py::test_full_gotoh_range_fuzz)
# ---------------------------------------------------------------------------------------------
# the algorithm flags the host rules read, as the C-ABI numbers them
F_NO_UNGAPPED, F_NO_PACKED, F_FORCE_PACKED, F_PK_STRIPE8, F_NO_NARROW, F_NO_COOP = 1, 4, 8, 256, 512, 32768

# neighbours differ, also round the end of the cycle (two jobs share a lane of the packed kernels); 7 of 17 are extreme (all-mismatch,
# perfect, shifted to the window's last diagonal), 5 of 17 ordinary mutated reads; the first 15 hold 7 and 4
FULL_KINDS = ("allmm", "mut", "perfect", "gap", "mut", "allmm", "shift", "mutn", "perfect", "gap", "mut", "random", "allmm", "mut", "shift",
              "gap", "mut")
FULL_GAPS = (1, 15, 40)


def full_step(sv):
    """the scheme's largest single term in absolute value, the match bonus among them"""
    return max(abs(int(v)) for v in sv)


def full_job(rng, kind, M, N, variant=0, allow_n=True):
    """one (pattern as aligned, text window) pair for a pattern of M symbols in a window of N -> (pattern, text, kind): a window shorter
    than its read holds no kind but an unrelated read ('short')"""
    if N < M or M == 0:
        return rng.integers(0, 4, M, dtype=np.uint8), rng.integers(0, 4, N, dtype=np.uint8), "short"
    txt = rng.integers(0, 4, N, dtype=np.uint8)
    if kind == "gap" and M < 4:
        kind = "random"                                              # (no neighbour of a gap job in FULL_KINDS is a random one)
    if kind == "allmm":                                              # the read is one letter, the text holds the other three
        a = int(rng.integers(0, 4))
        return np.full(M, a, dtype=np.uint8), ((a + 1 + rng.integers(0, 3, N)) % 4).astype(np.uint8), kind
    if kind == "perfect":
        d = int(rng.integers(0, N - M + 1))
        return txt[d:d + M].copy(), txt, kind
    if kind == "shift":                                              # the window's last diagonal: the sink is (N, M)
        return txt[N - M:].copy(), txt, kind
    if kind == "gap":                                                # one gap of 1, 15 or 40 symbols, in the pattern or in the text
        g = FULL_GAPS[variant % 3]
        in_text = (variant // 3) % 2 == 0 and N >= M + g             # the read lacks g symbols of the window
        if not in_text and M < g + 8:
            g = 1
            in_text = in_text and N >= M + 1
        p = (min(2, M - 2), M // 2, M - 2)[(variant // 6) % 3]
        if in_text:
            d = int(rng.integers(0, N - M - g + 1))
            return np.concatenate([txt[d:d + p], txt[d + p + g:d + g + M]]), txt, kind
        p = max(min(p, M - g - 2), 1)
        d = int(rng.integers(0, N - (M - g) + 1))
        return np.concatenate([txt[d:d + p], rng.integers(0, 4, g, dtype=np.uint8), txt[d + p:d + M - g]]), txt, kind
    if kind == "random":
        return rng.integers(0, 4, M, dtype=np.uint8), txt, kind
    d = int(rng.integers(0, N - M + 1))                              # mut, mutn: 0-5 substitutions and (M > 12) an indel of 1-3 symbols
    src = np.concatenate([txt[d:], rng.integers(0, 4, 4, dtype=np.uint8)])
    if M > 12:
        p = int(rng.integers(1, M - 4)); g = int(rng.integers(1, 4))
        r = (np.concatenate([src[:p], src[p + g:]]) if rng.random() < 0.5 else
             np.concatenate([src[:p], rng.integers(0, 4, g, dtype=np.uint8), src[p:]]))[:M]
    else:
        r = src[:M]
    r = _substitute(rng, r.copy(), int(rng.integers(0, 6)))
    if kind == "mutn":
        k = int(rng.integers(1, 4))
        if allow_n:
            r[rng.integers(0, M, k)] = 4
        else:
            _substitute(rng, r, k)
    return r, txt, kind


def full_jobs(seed, shapes, first=0, allow_n=True, kinds=None):
    """jobs of the given (M, N) shapes, job j of kind FULL_KINDS[(first + j) % 17] (or kinds[j]) -> (patterns, texts, kind names)"""
    rng = np.random.default_rng(seed)
    pats, txts, names, seen = [], [], [], {}
    for j, (M, N) in enumerate(shapes):
        kind = kinds[j] if kinds is not None else FULL_KINDS[(first + j) % len(FULL_KINDS)]
        v = seen.get(kind, 0); seen[kind] = v + 1
        p, t, kind = full_job(rng, kind, int(M), int(N), v + first, allow_n)
        assert len(p) == M and len(t) == N and p.dtype == np.uint8 and t.dtype == np.uint8
        pats.append(p); txts.append(t); names.append(kind)
    return pats, txts, np.array(names)


def full_shapes(seed, M, N, n, dominant=2, of=3, min_text=0):
    """n shapes: `dominant` of every `of` jobs have the batch's shape (M, N), the others a pattern of 1..M symbols in a window of
    min_text..N; every 16th of those windows is shorter than its read and every 40th empty (they report nothing)"""
    rng = np.random.default_rng(seed)
    shapes, odd = [], 0
    for j in range(n):
        if j % of < dominant:
            shapes.append((M, N))
            continue
        m = int(rng.integers(1, M + 1))
        w = int(rng.integers(max(min_text, m), max(N, m) + 1)) if N >= m else N
        if min_text == 0 and odd % 16 == 7:
            w = int(rng.integers(0, m)) if odd % 40 != 39 else 0
        odd += 1
        shapes.append((m, min(w, N)))
    return shapes


def _band31_int16_ok(sv, M):
    """packed_ok( SEMI_GLOBAL, ... ) of csrc/band31_packed.hip: what the narrow route asks of the band-31 kernel it borrows"""
    match, lim = sv[0], 4096
    pen = (sv[1], sv[2], -sv[3], -sv[4], -sv[5], -sv[6])
    return M > 0 and match >= 0 and all(0 <= v <= lim for v in pen) and (M + 32) * max(max(pen), match) <= 8000


def full_route(typ, sv, blocking, M, N, n, algo=0, has_min_scores=False, read_bits=4, text_bits=2, has_quals=False):
    """which kernel nvbio_full_gotoh_score gives the DP of a batch of n jobs declared as max_pattern_len = M, max_text_len = N: 'coop',
    'pk' (two jobs per lane, 8 columns per stripe), 'pk16' (the end-to-end build, 16 columns) or 'i32', behind 'narrow+' where the
    band-31 route runs in front -- full_score() and full_packed_ok() of csrc/gotoh_full.hip restated.  Only the jobs of shape (M, N) of
    a 'pk' batch run packed"""
    match, mm_min, mm_max, pat_go, pat_ge, txt_go, txt_ge = (int(v) for v in sv)
    step = full_step(sv)
    pk_bits = text_bits == 2 and read_bits in (2, 4)
    wanted = (n >= 262144 or bool(algo & F_FORCE_PACKED)) and not algo & F_NO_PACKED and not blocking
    e2e = typ == _SEMI_GLOBAL and match == 0 and not algo & F_NO_UNGAPPED
    if (typ in (_GLOBAL, _SEMI_GLOBAL) and not e2e and not wanted and not has_min_scores and pk_bits and 1 <= M <= 256
            and (M + N + 2) * step <= 30000 and not algo & F_NO_COOP):
        return "coop"
    shortcut = (e2e and pk_bits and mm_min >= 0 and mm_max >= 0 and (not has_quals or mm_min == mm_max)
                and pat_go < 0 and txt_go < 0 and pat_ge <= 0 and txt_ge <= 0)
    terms_ok = match >= 0 and all(v >= 0 for v in (mm_min, mm_max, -pat_go, -pat_ge, -txt_go, -txt_ge))
    packed = (wanted and pk_bits and M > 0 and N > 0 and terms_ok and step <= 4096 and (M + N) * step <= 12000
              and (typ != _LOCAL or match * M <= 2000))
    narrow = shortcut and not blocking and not algo & (F_NO_NARROW | F_NO_PACKED) and M <= 161 and _band31_int16_ok(sv, M) and pat_ge < 0
    dp = "i32" if not packed else "pk16" if typ == _SEMI_GLOBAL and match == 0 and not algo & F_PK_STRIPE8 else "pk"
    return ("narrow+" if narrow else "") + dp


def full_last_admitted(route, typ, sv, M=None):
    """the last max_text_len the rule of `route` admits at max_pattern_len = M; with M = None the last max_pattern_len of the rules that
    bound the pattern alone: LOCAL's sink key for 'pk' (match * M <= 2000), the cooperative kernel's 256 rows, the narrow route's 161"""
    step = full_step(sv)
    if route in ("pk", "pk16"):
        return 2000 // sv[0] if M is None else 12000 // step - M
    if route == "coop":
        return 256 if M is None else 30000 // step - M - 2
    if route == "narrow":
        return min(161, 8000 // step - 32)
    return None


def full_layout(pats, txts, quals=None, flags=None):
    """range_layout() plus what the oracle's batch call takes: the patterns as aligned, one after another, and the offsets of both"""
    L = range_layout(pats, txts, quals, flags)
    L["pats"] = np.concatenate(pats)
    L["pquals"] = np.concatenate(quals) if quals is not None else None
    L["toffs"] = np.concatenate([L["wb"], L["we"][-1:]]).astype(np.uint32)
    L["M"] = np.array([len(p) for p in pats], dtype=np.int64)
    L["N"] = np.array([len(t) for t in txts], dtype=np.int64)
    return L


# the edges of the packed route: (name, type, scheme, max_pattern_len or None for LOCAL's key rule, base qualities?)
FULL_PK_EDGES = (
    ("g_flat8_m9", _GLOBAL, flat_scheme(0, 8), 9, False),
    ("g_flat8_m24", _GLOBAL, flat_scheme(0, 8), 24, False),
    ("g_match8_flat8_m24", _GLOBAL, flat_scheme(8, 8), 24, False),
    ("g_flat40_m9", _GLOBAL, flat_scheme(0, 40), 9, False),
    ("g_flat1_m9", _GLOBAL, flat_scheme(0, 1), 9, False),
    ("g_flat4096_m1", _GLOBAL, flat_scheme(0, 4096), 1, False),                  # M + N = 2 | 3
    ("g_penalty4096_m1", _GLOBAL, flat_scheme(0, 4096), 1, False),               # the other side is a penalty of 4097
    ("g_asym8_m24", _GLOBAL, (2, 5, 5, -8, -2, -6, -3), 24, False),
    ("sg_flat8_m24", _SEMI_GLOBAL, flat_scheme(0, 8), 24, False),                # match 0: the end-to-end build, 16 columns
    ("sg_flat8_m9", _SEMI_GLOBAL, flat_scheme(0, 8), 9, False),
    ("sg_match3_flat8_m9", _SEMI_GLOBAL, flat_scheme(3, 8), 9, False),
    ("sg_ramp8_m24", _SEMI_GLOBAL, (0, 2, 8, -8, -3, -8, -3), 24, True),
    ("l_flat8_m24", _LOCAL, flat_scheme(2, 8), 24, False),
    ("l_key_match2", _LOCAL, (2, 3, 3, -5, -2, -5, -2), None, False),             # M = 1000 | 1001
    ("l_key_match1", _LOCAL, (1, 2, 2, -2, -1, -2, -1), None, False),             # M = 2000 | 2001
    ("l_key_match20", _LOCAL, (20, 6, 6, -8, -3, -8, -3), None, False),           # M = 100 | 101
    ("l_key_match5_ramp", _LOCAL, (5, 2, 6, -5, -3, -7, -2), None, True),         # M = 400 | 401
)


def full_pk_edge_sides(edge):
    """an edge of FULL_PK_EDGES -> ((scheme, M, N) last admitted, (scheme, M, N) first refused) under NVBIO_ALN_FORCE_PACKED_DP: the
    next window length; for LOCAL's key rule the next pattern length in a window of M + 40; for the penalty limit the next penalty"""
    name, typ, sv, M, _ = edge
    if M is None:
        M = full_last_admitted("pk", typ, sv)
        return ((sv, M, M + 40), (sv, M + 1, M + 41))
    N = full_last_admitted("pk", typ, sv, M)
    if "penalty" in name:
        return ((sv, M, N), (tuple(v + (1 if v > 0 else -1) if abs(v) == 4096 else v for v in sv), M, N))
    return ((sv, M, N), (sv, M, N + 1))


# ---------------------------------------------------------------------------------------------
# inputs for the banded traceback at the limits of its routes (tests/test_gpu_traceback_routes.py,
# tests/test_oracle_vs_reference.py::test_traceback_limit_fuzz)
# ---------------------------------------------------------------------------------------------
# (name, scheme, base qualities?): equal gap kinds; the text gap cheaper and its mirror (go_min / ge_min come from the cheaper kind); a
# quality ramp (a mismatch costs 2 to 6: the plane count stands aside); one the narrow route must refuse (match bonus 1)
LIMIT_SCHEMES = (
    ("equal", (0, 6, 6, -8, -3, -8, -3), False),
    ("cheap_txt", (0, 6, 6, -11, -4, -6, -2), False),
    ("cheap_pat", (0, 6, 6, -6, -2, -11, -4), False),
    ("ramp", (0, 2, 6, -8, -3, -8, -3), True),
    ("refused", (1, 3, 3, -8, -3, -8, -3), False),
)
LIMIT_M = 64                                                         # the read length of the bulk of the jobs
LIMIT_READ_LENS = (33, 64, 160, 161, 162)                            # 161 | 162: the plane count's limit; 33: an 8-symbol gap with clean flanks
LIMIT_WINDOWS = (31, 30, 29)                                         # window = M + this: M + 29 is the first the narrow routes refuse
LIMIT_GAP_KINDS = ("del", "ins", "del+sub", "ins+sub", "split")
LIMIT_FILLS = (3, 0, 4)                                              # what an overhang holds: the sentinel's low bits, another letter, N
LIMIT_SUB_QUALS = (0, 63, 10)                                        # the substituted symbol's quality: a ramp (2..6) charges 2, 6, 3


def _limit_path(rng, txt, M, d0, steps, front=None):
    """the read that follows `txt` from diagonal d0 on through `steps` = [("D", a) | ("I", b), ...] (D: the read lacks a text symbols, the
    diagonal moves up; I: b symbols more in the read, it moves down), 6 to 8 clean symbols in front of each (`front` of them in front of the
    first, when given: the read column the first gap starts at) and 7 or more behind the last
    -> (read, last diagonal, read positions free for a substitution)"""
    read, t, free = [], d0, []
    room = M - sum(n for k, n in steps if k == "I")
    flank = max(6, min(8, (room - 7) // len(steps))) if steps else 0
    for i, (k, n) in enumerate(steps):
        f = int(rng.integers(6, flank + 1)) if flank > 6 else 6
        if i == 0 and front is not None:
            f = front
        free += list(range(len(read) + 2, len(read) + f - 2))
        read += list(txt[t:t + f]); t += f
        if k == "D":
            t += n
        else:                                                        # inserted symbols differ from the text symbol the first would meet
            ins = rng.integers(0, 4, n)
            ins[0] = (int(txt[t]) + 1 + int(rng.integers(0, 3))) % 4
            read += list(ins)
    rest = M - len(read)
    assert rest >= 7 or not steps, (M, steps)
    free += list(range(len(read) + 2, M - 2))
    read += list(txt[t:t + rest]); t += rest
    assert len(read) == M and t <= len(txt)
    return np.array(read, dtype=np.uint8), t - M, free


def limit_jobs(seed):
    """jobs built so that the intended alignment of each ends on a chosen diagonal e of band 31, deterministic from the seed -> dict of
    per-job lists / arrays: pats (as aligned), txts (the window), quals, kind, e, L (gap symbols; substitutions of an ungapped job; overhang
    symbols), M, win (window length - M), fill (overhang jobs, else -1).

      del, ins            one gap of L = 1..8 symbols ending on e = 0..30, wherever the path stays inside columns 0..30
      del+sub, ins+sub    the same with one substitution (its quality cycles through LIMIT_SUB_QUALS)
      split               the gap as two of opposite kind, L = a + b, in both orders
      ungapped            0..3 substitutions on every e
      overhang            a read that matches the last M - L symbols of a window clipped by the text's end on diagonal e (window = e + M - L
                          symbols) and then holds L = 1..5 more: all 3, all 0 or all N.  e in {0, 15, 29, 30} and e = L, the lowest diagonal
                          whose window still holds the read (at e = 0 it does not: nothing is reported)
    The bulk has M = LIMIT_M in windows of M + 31; every third gap job comes again in windows of M + 30 and M + 29, every fourth at each other
    read length of LIMIT_READ_LENS."""
    rng = np.random.default_rng(seed)
    J = dict(pats=[], txts=[], quals=[], kind=[], e=[], L=[], M=[], win=[], fill=[])
    nsub = [0]

    def add(kind, pat, txt, e, L, M, win, fill=-1, subs=()):
        q = rng.integers(0, 64, M, dtype=np.uint8)
        for p in subs:
            q[p] = LIMIT_SUB_QUALS[nsub[0] % 3]; nsub[0] += 1
        for key, v in zip(("pats", "txts", "quals", "kind", "e", "L", "M", "win", "fill"), (pat, txt, q, kind, e, L, M, win, fill)):
            J[key].append(v)

    def gap_jobs(M, win, pick):
        for e in range(31):
            for L in range(1, 9):
                if not pick(e, L):
                    continue
                plans = [("del", [("D", L)], e - L), ("ins", [("I", L)], e + L)]
                if L > 1:
                    a = e % (L - 1) + 1; b = L - a
                    plans += [("split", [("D", a), ("I", b)], e + b - a), ("split", [("I", a), ("D", b)], e - b + a)]
                for kind, steps, d0 in plans:
                    d, inside = d0, 0 <= d0 <= 30
                    for k, n in steps:
                        d += n if k == "D" else -n
                        inside = inside and 0 <= d <= 30
                    if not inside or e + M > M + win:                # (the path leaves the band, or the window)
                        continue
                    for sub in ((0, 1) if kind != "split" else (0,)):
                        txt = rng.integers(0, 4, M + win, dtype=np.uint8)
                        pat, end, free = _limit_path(rng, txt, M, d0, steps)
                        assert end == e
                        subs = ()
                        if sub:
                            p = int(free[int(rng.integers(0, len(free)))])
                            pat[p] = (pat[p] + 1 + rng.integers(0, 3)) % 4; subs = (p,)
                        add(kind + ("+sub" if sub else ""), pat, txt, e, L, M, win, subs=subs)

    gap_jobs(LIMIT_M, 31, lambda e, L: True)
    for win in LIMIT_WINDOWS[1:]:
        gap_jobs(LIMIT_M, win, lambda e, L: (e + L) % 3 == 0 or e >= 29)
    for i, M in enumerate(m for m in LIMIT_READ_LENS if m != LIMIT_M):
        gap_jobs(M, 31, lambda e, L: (e * 8 + L) % 4 == i)
    for M in (LIMIT_M, 161, 162):
        for e in range(31):
            for s in range(4):
                txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                pat = txt[e:e + M].copy()
                subs = tuple(int(p) for p in rng.choice(M, s, replace=False))
                for p in subs:
                    pat[p] = (pat[p] + 1 + rng.integers(0, 3)) % 4
                add("ungapped", pat, txt, e, s, M, 31, subs=subs)
    M = LIMIT_M
    for k in range(1, 6):
        for e in (0, k, 15, 29, 30):
            for fill in LIMIT_FILLS:
                txt = rng.integers(0, 4, e + M - k, dtype=np.uint8)
                txt[-1] = (fill + 1) % 4 if fill < 4 else txt[-1]     # (the text's last symbol is not the overhang's: the diagonal's matches end there)
                pat = np.concatenate([txt[e:], np.full(k, fill, dtype=np.uint8)])
                add("overhang", pat, txt, e, k, M, e - k, fill=fill)
    for key in ("kind", "e", "L", "M", "win", "fill"):
        J[key] = np.array(J[key])
    return J


def limit_select(J, idx):
    """the jobs `idx` of limit_jobs()' result"""
    idx = np.asarray(idx)
    return {k: ([v[i] for i in idx] if isinstance(v, list) else v[idx]) for k, v in J.items()}


def limit_thin(J):
    """one job of every (kind, read length, window length, overhang fill and diagonal) of limit_jobs()' result -- of every (kind, read length,
    window length, fill, gap column) of full_limit_jobs()' --, from the middle of each group"""
    groups = {}
    win = J["win"] if "win" in J else J["W"]
    for j in range(len(J["kind"])):
        over = J["kind"][j] == "overhang"
        key = (J["kind"][j], int(J["M"][j]), int(win[j]) if not over else int(J["e"][j]), int(J["fill"][j]))
        groups.setdefault(key + ((int(J["col"][j]),) if "col" in J else ()), []).append(j)
    return np.array(sorted(g[len(g) // 2] for g in groups.values()))


# ---------------------------------------------------------------------------------------------
# inputs for the full-matrix traceback at the limits of its routes (tests/test_full_traceback_limit_jobs.py,
# tests/test_gpu_full_traceback_routes.py, tests/test_oracle_vs_reference.py::test_full_traceback_limit_fuzz)
# ---------------------------------------------------------------------------------------------
FULL_LIMIT_WINDOWS = (13, 14, 15, 22, 40)                            # window = M + this: M + 14 is the first the band route takes
FULL_LIMIT_COLS = (7, 8, 9, 15, 16, 17, 30)                          # the read column a gap starts at: on, before and behind a stripe boundary
FULL_LIMIT_READ_LENS = (1, 7, 8, 9, 16, 17, 33, 64, 65)
FULL_LIMIT_SHORT_K = (1, 7, 8, 9)                                    # short texts: N = M - k
FULL_LIMIT_CUT_SCHEME = ("cut", (0, 3, 3, -1, -1, -1, -1), False)    # go_min = ge_min = 1: G = -best, the cut G <= 250 | 251 at M = 250 | 251
FULL_LIMIT_CUT_LENS = (249, 250, 251, 252)
FULL_LIMIT_MARGIN = 64                                               # text in front of the first window and behind the last
ALN_NO_UNGAPPED_TRACEBACK, ALN_NO_NARROW_TRACEBACK, ALN_NO_BAND_ROUTE = 16, 64, 1024    # NVBIO_ALN_* of include/nvbio_amd.h


def full_limit_jobs(seed):
    """jobs built so that the intended alignment of each ends on a chosen sink diagonal `delta` = sink.x - sink.y of a window of M + W
    symbols, deterministic from the seed -> dict of per-job lists / arrays as limit_jobs(): pats (as aligned), txts (the window), quals, kind,
    delta, L (gap symbols; substitutions of an ungapped job; the k of a short text), M, W (= N - M), fill (4: the read holds an N, else -1),
    col (the read column the first gap starts at, else -1).

      del, ins            one gap of L = 1..12 symbols ending on delta, wherever the path stays on diagonals 0..W; M = LIMIT_M; W in
                          FULL_LIMIT_WINDOWS with every delta (W = 40: 0..9, 19, 20, 31..40); col cycles through FULL_LIMIT_COLS per kind
      del+sub, ins+sub    the same with one substitution (its quality cycles through LIMIT_SUB_QUALS)
      split               the gap as two of opposite kind, L = a + b, in both orders
      lens                reads of FULL_LIMIT_READ_LENS: ungapped or with one substitution; from 16 symbols on with one gap of 1, 2, 3 or 8 as
                          well, from 7 to 9 with a deletion of one symbol (for the restricted rows and the band: a lone substitution is settled)
      ungapped            0..3 substitutions at every delta of W = 15 and W = 40; every seventh read holds an N
      short               N = M - k for k in FULL_LIMIT_SHORT_K, and N = 1: the read is the text and k more symbols behind it ("short") or
                          in front ("short_lead"); sink.x < sink.y, delta = -k
      cut                 reads of FULL_LIMIT_CUT_LENS symbols 0 in windows of M + 20 that hold no 0: three letters, and two letters"""
    rng = np.random.default_rng(seed)
    keys = ("pats", "txts", "quals", "kind", "delta", "L", "M", "W", "fill", "col")
    J = {k: [] for k in keys}
    nsub, ncol = [0], {}

    def add(kind, pat, txt, delta, L, M, W, fill=-1, col=-1, subs=()):
        q = rng.integers(0, 64, M, dtype=np.uint8)
        for p in subs:
            q[p] = LIMIT_SUB_QUALS[nsub[0] % 3]; nsub[0] += 1
        for key, v in zip(keys, (pat, txt, q, kind, delta, L, M, W, fill, col)):
            J[key].append(v)

    def gap_jobs(M, W, deltas, lens, cols, tag=None):
        for delta in deltas:
            for L in lens:
                plans = [("del", [("D", L)], delta - L), ("ins", [("I", L)], delta + L)]
                if L > 1:
                    a = delta % (L - 1) + 1; b = L - a
                    plans += [("split", [("D", a), ("I", b)], delta + b - a), ("split", [("I", a), ("D", b)], delta - b + a)]
                for kind, steps, d0 in plans:
                    d, inside = d0, 0 <= d0 <= W
                    for k, n in steps:
                        d += n if k == "D" else -n
                        inside = inside and 0 <= d <= W
                    if not inside:                                   # (the path leaves the window)
                        continue
                    for sub in ((0, 1) if kind != "split" else (0,)):
                        name = kind + ("+sub" if sub else "")
                        ins = sum(n for k, n in steps if k == "I")
                        fit = [c for c in cols if c + ins + 8 * (len(steps) - 1) + 7 <= M]
                        if not fit:
                            continue
                        col = fit[ncol.get((name, M), 0) % len(fit)]; ncol[(name, M)] = ncol.get((name, M), 0) + 1
                        txt = rng.integers(0, 4, M + W, dtype=np.uint8)
                        pat, end, free = _limit_path(rng, txt, M, d0, steps, front=col)
                        assert end == delta
                        subs = ()
                        if sub:
                            p = int(free[int(rng.integers(0, len(free)))])
                            pat[p] = (pat[p] + 1 + rng.integers(0, 3)) % 4; subs = (p,)
                        add(tag or name, pat, txt, delta, L, M, W, col=col, subs=subs)

    for W in FULL_LIMIT_WINDOWS:
        deltas = range(W + 1) if W != 40 else list(range(10)) + [19, 20] + list(range(31, 41))
        gap_jobs(LIMIT_M, W, deltas, range(1, 13), FULL_LIMIT_COLS)
    for M in FULL_LIMIT_READ_LENS:
        for W in (15, 22):
            for delta in (0, 6, 7, 8, W - 7, W - 6, W):
                for s in (0, 1):
                    txt = rng.integers(0, 4, M + W, dtype=np.uint8)
                    pat = txt[delta:delta + M].copy()
                    subs = tuple(int(p) for p in rng.choice(M, s, replace=False))
                    for p in subs:
                        pat[p] = (pat[p] + 1 + rng.integers(0, 3)) % 4
                    add("lens", pat, txt, delta, s, M, W, subs=subs)
        if 7 <= M < 16:                                              # (too short for _limit_path's flanks: one text symbol skipped mid-read)
            for W in (15, 22):
                for d0 in (0, 5, 6, 7, W - 8, W - 7, W - 1):
                    txt = rng.integers(0, 4, M + W, dtype=np.uint8)
                    c = M // 2
                    add("lens", np.concatenate([txt[d0:d0 + c], txt[d0 + c + 1:d0 + M + 1]]), txt, d0 + 1, 1, M, W, col=c)
        if M >= 16:
            gap_jobs(M, 22, (0, 3, 7, 8, 11, 15, 19, 22), (1, 2, 3, 8), FULL_LIMIT_COLS, tag="lens")
    for W in (15, 40):
        for delta in range(W + 1):
            for s in range(4):
                txt = rng.integers(0, 4, LIMIT_M + W, dtype=np.uint8)
                pat = txt[delta:delta + LIMIT_M].copy()
                subs = tuple(int(p) for p in rng.choice(LIMIT_M, s, replace=False))
                for p in subs:
                    pat[p] = (pat[p] + 1 + rng.integers(0, 3)) % 4
                fill = -1
                if len(J["pats"]) % 7 == 0:
                    pat[int(rng.integers(0, LIMIT_M))] = 4; fill = 4
                add("ungapped", pat, txt, delta, s, LIMIT_M, W, fill=fill, subs=subs)
    for M, N in [(LIMIT_M, LIMIT_M - k) for k in FULL_LIMIT_SHORT_K] + [(20, 10), (LIMIT_M, 1), (9, 1), (33, 24)]:
        for rep in range(4):
            txt = rng.integers(0, 4, N, dtype=np.uint8)
            more = rng.integers(0, 4, M - N, dtype=np.uint8)       # (its ends differ from the text's: the insertions cannot slide inwards)
            more[-1] = (txt[-1] + 1 + rng.integers(0, 3)) % 4 if more[-1] == txt[-1] else more[-1]
            more[0] = (txt[0] + 1 + rng.integers(0, 3)) % 4 if more[0] == txt[0] else more[0]
            add("short", np.concatenate([txt, more]), txt, N - M, M - N, M, N - M)
            add("short_lead", np.concatenate([more, txt]), txt, N - M, M - N, M, N - M)
    for M in FULL_LIMIT_CUT_LENS:
        for letters in ((1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 3)):
            txt = rng.choice(np.array(letters, dtype=np.uint8), M + 20)
            add("cut", np.zeros(M, dtype=np.uint8), txt, 20, M, M, 20)
    for key in keys[3:]:
        J[key] = np.array(J[key])
    return J


def full_limit_layout(J, with_q, flags=None):
    """full_layout() of full_limit_jobs()' jobs (or a limit_select() of them), the windows inside one text with FULL_LIMIT_MARGIN symbols in
    front of the first and behind the last: a window rule that is off by one reads text, never memory outside the buffer"""
    L = full_layout(J["pats"], J["txts"], J["quals"] if with_q else None, flags)
    m = (np.arange(FULL_LIMIT_MARGIN) % 4).astype(np.uint8)
    L["text"] = np.concatenate([m, L["text"], m[::-1]])
    for key in ("wb", "we", "toffs"):
        L[key] = (L[key] + FULL_LIMIT_MARGIN).astype(np.uint32)
    return L


def full_limit_oracle(orc, typ, sv, J, with_q, stride, min_scores=None):
    """orc.full_gotoh_traceback job by job -> (scores, sources, sinks, cigars[n, stride], lens) as the GPU entry point lays them out: the
    CIGAR's elements beyond `stride` dropped, its length not"""
    import oracle
    n = len(J["pats"])
    sc = oracle.Scheme(*sv)
    scores = np.zeros(n, dtype=np.int32); lens = np.zeros(n, dtype=np.uint32)
    sources = np.zeros((n, 2), dtype=np.uint32); sinks = np.zeros((n, 2), dtype=np.uint32)
    cigars = np.zeros((n, stride), dtype=np.uint16)
    for j in range(n):
        ms = oracle.SCORE_MIN if min_scores is None else int(min_scores[j])
        ok, s, src, snk, cig = orc.full_gotoh_traceback(typ, sc, J["pats"][j], J["txts"][j], J["quals"][j] if with_q else None, ms)
        scores[j], sources[j], sinks[j], lens[j] = s, src, snk, len(cig)
        cigars[j, :min(len(cig), stride)] = cig[:stride]
    return scores, sources, sinks, cigars, lens


def full_gap_mins(sv):
    """the cheapest gap opening / extension penalty of a scheme (narrow_e2e's go_min, ge_min)"""
    return -max(sv[3], sv[5]), -max(sv[4], sv[6])


def full_gap_bound(a, sv):
    """e2e_gap_bound of the cost a = -best"""
    go, ge = full_gap_mins(sv)
    return 0 if a < go else (a - go) // ge + 1


def full_narrow_scheme(typ, sv):
    """narrow_e2e without the algo flag"""
    go, ge = full_gap_mins(sv)
    return typ == _SEMI_GLOBAL and sv[0] == 0 and sv[1] >= 0 and sv[2] >= 0 and ge > 0 and go >= ge


def _full_diagonal_settles(pat, q, txt, typ, sv, best, sink):
    """ungapped_full_traceback_kernel's walk: do the k diagonal steps that end in `sink` score `best` -- SEMI_GLOBAL: k = sink.y, which needs
    sink.x >= sink.y; LOCAL: some k <= min(sink.x, sink.y), or best == 0; GLOBAL: never"""
    x, y = int(sink[0]), int(sink[1])
    if typ == _GLOBAL or (typ == _SEMI_GLOBAL and x < y):
        return False
    k = min(x, y)
    p = pat[y - k:y].astype(np.int64)
    g = txt[x - k:x].astype(np.int64)
    qq = np.minimum(q[y - k:y].astype(np.int64), 40) if q is not None else np.zeros(k, dtype=np.int64)
    mm = sv[1] + (qq.astype(np.float32) / np.float32(40) * np.float32(sv[2] - sv[1])).astype(np.int64)
    step = np.where(g == p, sv[0], -mm)
    if typ == _LOCAL:
        return best == 0 or bool((np.cumsum(step[::-1]) == best).any())
    return k == y and int(step.sum()) == best


def full_route_rule(J, with_q, typ, sv, want, algo=0):
    """(routes, gap_bound) of every job of nvbio_full_gotoh_traceback_routes, restated from the conditions of csrc/gotoh_full_traceback.hip
    on the oracle's score and sink (`want` as full_limit_oracle() returns it): 0 where nothing is traced or the sink's diagonal settles the job;
    else 1, or under a scheme narrow_e2e admits, with the sink in the last pattern row, best <= 0 and G = e2e_gap_bound(best) <= 250: 2 with
    gap_bound G -- 3 where also G <= 7, sink.x >= sink.y, N >= M + 14 and 7 <= delta <= N - M - 7"""
    n = len(J["pats"])
    routes, bound = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    if algo & ALN_NO_UNGAPPED_TRACEBACK:
        return routes + 1, bound
    narrow = full_narrow_scheme(typ, sv) and not algo & ALN_NO_NARROW_TRACEBACK
    band = narrow and not algo & ALN_NO_BAND_ROUTE
    sc, sk = want[0], want[2].astype(np.int64)
    for j in range(n):
        M, N = len(J["pats"][j]), len(J["txts"][j])
        if want[4][j] == 0 or _full_diagonal_settles(J["pats"][j], J["quals"][j] if with_q else None, J["txts"][j], typ, sv, int(sc[j]), sk[j]):
            continue
        routes[j] = 1
        if narrow and sk[j, 1] == M and sc[j] <= 0:
            G = full_gap_bound(-int(sc[j]), sv)
            if G <= 250:
                routes[j], bound[j] = 2, G
                delta = int(sk[j, 0] - sk[j, 1])
                if band and G <= 7 and sk[j, 0] >= sk[j, 1] and N >= M + 14 and delta >= 7 and delta + 7 <= N - M:
                    routes[j] = 3
    return routes, bound


# ---------------------------------------------------------------------------------------------
# the band-31 end-to-end shortcuts over the scheme space (tests/test_e2e31_sweep_jobs.py, tests/test_gpu_band31_scheme_sweep.py,
# tests/test_oracle_vs_reference.py::test_e2e31_scheme_sweep)
# ---------------------------------------------------------------------------------------------
BAND31, NARROW_HALF_A, NARROW_HALF_B = 31, 6, 8                      # the narrow classes' half-widths (csrc/band31_jobs.h)
ALN_NO_UNGAPPED_SCORE, ALN_NO_THIRD_CHANCE, ALN_PK_THREE_WAVES, ALN_NO_SECOND_CHANCE = 1, 2, 32, 128    # NVBIO_ALN_* of include/nvbio_amd.h
ALN_NO_QUALITY_SHORTCUT, ALN_RAGGED_READS, ALN_NO_F16_DP, ALN_NO_GAP_CHANCE = 2048, 4096, 16384, 65536
ALN_SPLIT_CHANCES, ALN_NO_PAIRED_GAP_CHANCE, ALN_NO_NARROW_DP = 131072, 262144, 524288


def reach(L, go, ge):
    """r(L): the largest delta with go + (delta - 1) ge >= L (0: not even one column)"""
    d = 0
    while d < 64 and go + d * ge >= L:
        d += 1
    return d


def classes(cnt, P, go, ge):
    """per job (U*, best_d, class) from the 31 diagonals' mismatch counts: 0 none, 1 = B, 2 = A"""
    best = cnt.min(axis=1)
    best_d = (BAND31 - 1) - np.argmin(cnt[:, ::-1], axis=1)         # ties: the larger column, as BestSink
    U = -P * best
    w = np.array([reach(int(u), go, ge) for u in U]) + np.abs(best_d - 15)
    return U, best_d, np.where(w <= NARROW_HALF_A, 2, np.where(w <= NARROW_HALF_B, 1, 0))


def _sweep_grid():
    out = []
    for P in (0, 1, 2, 3, 6, 30):
        for go in (1, 2, 5, 8, 40):
            for ge in sorted({0, 1, 3, go, go + 2}):
                out.append((0, P, P, -go, -ge, -go, -ge))
    return tuple(out)


# every (P, |go|, |ge|) of P in {0, 1, 2, 3, 6, 30} x |go| in {1, 2, 5, 8, 40} x |ge| in {0, 1, 3, |go|, |go| + 2}: 138 symmetric schemes
E2E31_SWEEP = _sweep_grid()

# (name, scheme, base qualities?): one or more per regime of the three numbers the shortcuts' arguments rest on
E2E31_CORNERS = (
    ("p0", (0, 0, 0, -5, -3, -5, -3), False),                        # a mismatch costs nothing: every diagonal scores 0
    ("p0_linear", (0, 0, 0, -2, -2, -2, -2), False),
    ("ge0", (0, 6, 6, -8, 0, -8, 0), False),                         # a gap costs its opening whatever its length
    ("ge0_p1", (0, 1, 1, -5, 0, -5, 0), False),
    ("open_below_ext", (0, 6, 6, -2, -5, -2, -5), False),            # |go| < |ge|: the first gap symbol is the cheapest
    ("open_below_ext_p3", (0, 3, 3, -1, -3, -1, -3), False),
    ("open_below_ext_p1", (0, 1, 1, -2, -5, -2, -5), False),         # ... with a U* the second chance takes: two mismatches
    ("two_gaps_tie", (0, 2, 2, -1, -3, -1, -3), False),              # P = 2 |G|: two gaps of one symbol tie a diagonal with one mismatch
    ("edit_distance", (0, 1, 1, -1, -1, -1, -1), False),             # go == ge == -P
    ("linear_p_below", (0, 1, 1, -3, -3, -3, -3), False),
    ("linear_p_above", (0, 5, 5, -2, -2, -2, -2), False),
    ("p30_cheap_gaps", (0, 30, 30, -2, -1, -2, -1), False),          # five gaps cost less than one mismatch
    ("p1_dear_gaps", (0, 1, 1, -40, -3, -40, -3), False),            # cap = 120
    ("pinned_6_8_3", (0, 6, 6, -8, -3, -8, -3), False),              # the six the route tests held before this sweep
    ("pinned_2_5_1", (0, 2, 2, -5, -1, -5, -1), False),
    ("pinned_4_6_6", (0, 4, 4, -6, -6, -6, -6), False),
    ("pinned_3_4_2", (0, 3, 3, -4, -2, -4, -2), False),
    ("pinned_6_5_3", (0, 6, 6, -5, -3, -5, -3), False),
    ("pinned_3_3_3_txt_9_1", (0, 3, 3, -3, -3, -9, -1), False),
    ("cheap_txt", (0, 6, 6, -11, -4, -6, -2), False),                # asymmetric: G comes from the text gap, the recurrences' terms from the pattern gap
    ("cheap_pat", (0, 6, 6, -6, -2, -11, -4), False),
    ("ramp_2_6", (0, 2, 6, -8, -3, -8, -3), True),
    ("ramp_1_7", (0, 1, 7, -8, -3, -8, -3), True),
    ("ramp_3_10", (0, 3, 10, -8, -3, -8, -3), True),
    ("ramp_0_6_no_quals", (0, 0, 6, -8, -3, -8, -3), False),         # without qualities every mismatch costs mm_min = 0
)
E2E31_SWEEP_M = (64, 161)                                            # the read lengths of what e2e31_sweep_jobs() adds to limit_jobs()
E2E31_SWEEP_DIAGONALS = (0, 7, 15, 23, 30)


def e2e31_sweep_jobs(seed):
    """limit_jobs(seed) and, at M = 64 and M = 161 in windows of M + 31, what that pool lacks -> the same dict (e: the diagonal the intended
    alignment ends on, L: gap symbols, or substitutions / N's of an ungapped job):

      subs            4..12 substitutions on diagonals 0, 7, 15, 23 and 30: spread over the read, clustered at its front, at its end
      gap+subs        one gap of 1..3 symbols and 2 or 3 substitutions
      gaps2, gaps3    two and three gaps of one symbol, every order of kinds
      longgap         one gap of 5, 6 or 9 symbols (the gap chance evaluates up to 5), alone and with one substitution
      periodic        reads on text of period 1, 2 and 3 with 0, 1, 2 and 4 substitutions: co-optimal alignments on every diagonal
      periodic_gap    a one-symbol gap inside a run of period 1, 2 or 3 in random text: the gap's placements tie
      n               reads with one N and with three N's, 0..2 substitutions beside them
      near_centre     4 and 5 substitutions on diagonals 13..17: the narrow classes' jobs at 0 / -6 / -8 / -3
      many_subs       M = 161 with 38..43 substitutions: second and third chance where a mismatch costs 1 and a gap 40
      allmm           a read of one letter in a window of the other three: beyond every cap"""
    J = limit_jobs(seed)
    J = {k: (list(v) if not isinstance(v, list) else v) for k, v in J.items()}
    rng = np.random.default_rng(seed + 7919)
    nsub = [0]

    def add(kind, pat, txt, e, L, M, subs=()):
        q = rng.integers(0, 64, M, dtype=np.uint8)
        for p in subs:
            q[p] = LIMIT_SUB_QUALS[nsub[0] % 3]; nsub[0] += 1
        for key, v in zip(("pats", "txts", "quals", "kind", "e", "L", "M", "win", "fill"), (np.asarray(pat, dtype=np.uint8), txt, q, kind, e, L, M, 31, -1)):
            J[key].append(v)

    def substitute(pat, pos):
        pos = np.asarray(pos, dtype=np.int64)
        pat[pos] = (pat[pos] + 1 + rng.integers(0, 3, len(pos))) % 4
        return tuple(int(p) for p in pos)

    for M in E2E31_SWEEP_M:
        for e in E2E31_SWEEP_DIAGONALS:
            for k in range(4, 13):
                for where in range(3):
                    txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                    pat = txt[e:e + M].copy()
                    pos = (rng.choice(M, k, replace=False), rng.choice(16, k, replace=False), M - 16 + rng.choice(16, k, replace=False))[where]
                    add("subs", pat, txt, e, k, M, substitute(pat, pos))
        for e in (4, 15, 26):
            for L in (1, 2, 3):
                for kind, d0 in (("D", e - L), ("I", e + L)):
                    for k in (2, 3):
                        txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                        pat, end, free = _limit_path(rng, txt, M, d0, [(kind, L)])
                        assert end == e
                        add("gap+subs", pat, txt, e, L, M, substitute(pat, rng.choice(free, k, replace=False)))
            for plan in ("DD", "DI", "ID", "II", "DDD", "DID", "IDI", "III"):
                d0 = e - plan.count("D") + plan.count("I")
                txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                pat, end, free = _limit_path(rng, txt, M, d0, [(k, 1) for k in plan])
                assert end == e
                add("gaps%d" % len(plan), pat, txt, e, len(plan), M)
        for e in (10, 15, 20):
            for L in (5, 6, 9):
                for kind, d0 in (("D", e - L), ("I", e + L)):
                    for k in (0, 1):
                        txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                        pat, end, free = _limit_path(rng, txt, M, d0, [(kind, L)])
                        assert end == e
                        add("longgap", pat, txt, e, L, M, substitute(pat, rng.choice(free, k, replace=False)))
        for e in E2E31_SWEEP_DIAGONALS:
            for period in (1, 2, 3):
                for k in (0, 1, 2, 4):
                    unit = rng.permutation(4)[:period].astype(np.uint8)
                    txt = np.resize(unit, M + 31)
                    pat = txt[e:e + M].copy()
                    add("periodic", pat, txt, e, k, M, substitute(pat, rng.choice(M, k, replace=False)))
        for e in (5, 15, 25):
            for period in (1, 2, 3):
                for kind in ("D", "I"):
                    txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                    d0 = e - 1 if kind == "D" else e + 1
                    at, run = M // 2, 24                             # the run covers rows at - 12 .. at + 12 of both diagonals
                    txt[min(d0, e) + at - 12:max(d0, e) + at + 12] = np.resize(rng.permutation(4)[:period].astype(np.uint8), run + 1)
                    pat = np.concatenate([txt[d0:d0 + at], txt[d0 + at + 1:d0 + M + 1]]) if kind == "D" else \
                        np.concatenate([txt[d0:d0 + at], txt[d0 + at - 1:d0 + at], txt[d0 + at:d0 + M - 1]])
                    assert len(pat) == M
                    add("periodic_gap", pat, txt, e, 1, M)
        for e in E2E31_SWEEP_DIAGONALS:
            for n_count in (1, 3):
                for k in (0, 1, 2):
                    txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                    pat = txt[e:e + M].copy()
                    pos = rng.choice(M, n_count + k, replace=False)
                    subs = substitute(pat, pos[n_count:])
                    pat[pos[:n_count]] = 4
                    add("n", pat, txt, e, n_count, M, subs)
        for e in (13, 14, 15, 16, 17):
            for k in (4, 5):
                for rep in range(6):
                    txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                    pat = txt[e:e + M].copy()
                    add("near_centre", pat, txt, e, k, M, substitute(pat, rng.choice(M, k, replace=False)))
        if M == 161:
            for e in E2E31_SWEEP_DIAGONALS:
                for k in range(38, 44):
                    for rep in range(2):
                        txt = rng.integers(0, 4, M + 31, dtype=np.uint8)
                        pat = txt[e:e + M].copy()
                        add("many_subs", pat, txt, e, k, M, substitute(pat, rng.choice(M, k, replace=False)))
        for a in range(4):
            for rep in range(2):
                txt = ((a + 1 + rng.integers(0, 3, M + 31)) % 4).astype(np.uint8)
                add("allmm", np.full(M, a, dtype=np.uint8), txt, 30, M, M)
    for key in ("kind", "e", "L", "M", "win", "fill"):
        J[key] = np.array(J[key])
    assert len(J["pats"]) < 6000
    return J


def e2e31_counts(J, with_q_scheme=None):
    """per job the 31 diagonals' mismatch counts, diagonal d = the read against the window from its symbol d on; -1 where the diagonal does not
    lie inside the window (it holds no reportable column).  An N differs from every symbol.  with_q_scheme = a scheme: the diagonals'
    penalty sums under its quality ramp instead (mismatch_score() of csrc/gotoh_common.h: mm_min + int( min(q, 40) / 40 * (mm_max - mm_min) )
    in binary32)"""
    n = len(J["pats"])
    out = np.full((n, BAND31), -1, dtype=np.int64)
    for j in range(n):
        pat, txt = J["pats"][j], J["txts"][j]
        M, N = len(pat), len(txt)
        w = np.ones(M, dtype=np.int64)
        if with_q_scheme is not None:
            lo, hi = with_q_scheme[1], with_q_scheme[2]
            q = np.minimum(J["quals"][j].astype(np.int64), 40)
            w = lo + (q.astype(np.float32) / np.float32(40) * np.float32(hi - lo)).astype(np.int64)
        for d in range(min(BAND31, N - M + 1)):
            out[j, d] = int(w[pat != txt[d:d + M]].sum())
    return out


def e2e31_admitted(sv, has_quals, max_read_len, algo=0):
    """does nvbio_banded_gotoh_score send a SEMI_GLOBAL band-31 batch of 4- or 2-bit reads on a 2-bit text through the shortcuts at all --
    packed_ok() of csrc/band31_packed.hip and ungapped_ok() of csrc/band31_stage.hip as the code has them"""
    match, mm_min, mm_max, pat_go, pat_ge, txt_go, txt_ge = (int(v) for v in sv)
    if algo & ALN_NO_UNGAPPED_SCORE or not _band31_int16_ok(sv, int(max_read_len)):
        return False
    if match != 0 or mm_min < 0 or mm_max < 0:
        return False
    if has_quals and mm_min != mm_max and (mm_min <= 0 or mm_max < mm_min or algo & ALN_NO_QUALITY_SHORTCUT):
        return False
    return pat_go < 0 and txt_go < 0 and pat_ge <= 0 and txt_ge <= 0 and mm_min > 0


def e2e31_classes_on(sv, has_quals, max_read_len, algo=0):
    """are the DP's narrow classes formed: narrow_rule() and its caller's condition (the binary16 DP follows, no qualities, not ragged)"""
    P, go, ge = int(sv[1]), int(sv[3]), int(sv[4])
    f16 = (not algo & (ALN_PK_THREE_WAVES | ALN_NO_F16_DP) and sv[0] == 0 and (int(max_read_len) + 32) * scheme_step(sv) <= 2040 and sv[2] <= 400)
    on = not has_quals and not algo & (ALN_NO_NARROW_DP | ALN_RAGGED_READS) and f16
    return bool(on and ge < 0 and P > 0 and go + NARROW_HALF_B * ge + 1 >= -2000)


def e2e31_first_pass(sv, has_quals, M, N, counts, weights=None, max_read_len=None, algo=0):
    """The first pass's rule AS THE CODE HAS IT (ungapped_e2e31_job, MODE 0, of csrc/band31_ungapped_inl.h), restated in numpy: this is a copy of
    the conditions, not a derivation of what they should be -- the tests hold the library's results to the oracle and its routes to this.
    From each job's read length M, window length N and 31 diagonal mismatch counts (e2e31_counts(): -1 off the window; under a quality ramp
    also `weights`, the diagonals' penalty sums) -> (flag, class) per job:

      flag 0  settled (U* > G, or nothing to report: N < M)       flag 3  second chance       flag 2  third chance       flag 4  gap chance
      flag 1  the DP, with its narrow class (0 none, 1 = B, 2 = A, as classes(); max_read_len decides whether classes are formed at all)

    With P = mm_min, go / ge the pattern gap's terms and G = max(pat_go, txt_go):
      floor_u = 3 min(G, go) - P, cap = the largest count with -P cnt > floor_u; cap_x = the largest count whose U* is still in class B, where
      that is larger, the classes are formed and the window is whole (N >= M + 30); best_cnt / best_d the fewest mismatches of a diagonal
      inside the window and the LAST diagonal that has them
      best_cnt > cap: class job if best_cnt <= cap_x and it has a class; else flag 4 if no ramp, P > 0, N >= M + 30, ge < 0, go <= ge; else DP
      U* = -P best_cnt (ramp: DP if U* <= 3 G - P, else U* = the largest penalty sum's negative among the diagonals with P cnt <= pmax best_cnt)
      U* > G: settled
      second_applies = G - P < U* and 2 G < U* and N >= M + 30, with gmax = the gap lengths 1..5 that reach U*, 1 <= gmax <= 4
      third_applies = N >= M + 30, not `beyond` (gmax0 > 4, gmax1 > 4, go - 2P, 2go + ge, 2go - P or 3go >= U*, ge < go), gmax0 >= 1 and
      (gmax1 >= 1 or 2 go >= U*)"""
    match, mm_min, mm_max, pat_go, pat_ge, txt_go, txt_ge = (int(v) for v in sv)
    P, go, ge, G = mm_min, pat_go, pat_ge, max(pat_go, txt_go)
    qual = bool(has_quals) and mm_min != mm_max
    M, N, counts = np.asarray(M, dtype=np.int64), np.asarray(N, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    n = len(M)
    flag, cls = np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    floor_u = 3 * min(G, go) - P
    cap = (-floor_u - 1) // P if P > 0 else 0xFFFFFFFE
    classes_on = max_read_len is not None and e2e31_classes_on(sv, has_quals, max_read_len, algo)
    cnt_max = (-(go + NARROW_HALF_B * ge + 1)) // P if classes_on else 0
    pmax = mm_min + int(np.float32(40) / np.float32(40) * np.float32(mm_max - mm_min))

    def span(base, U):                                               # how many of the gap lengths 1..5 reach U
        g = 0
        while g < 5 and base + g * ge >= U:
            g += 1
        return g

    def narrow(U, best_d):
        if not classes_on:
            return 0
        w = reach(int(U), go, ge) + abs(int(best_d) - 15)
        return 2 if w <= NARROW_HALF_A else 1 if w <= NARROW_HALF_B else 0

    for j in range(n):
        m, nn = int(M[j]), int(N[j])
        if nn < m:
            flag[j] = 0
            continue
        if m == 0 or m > 161:
            continue
        whole = nn >= m + 30
        on = counts[j] >= 0
        cap_x = cnt_max if (not qual and cnt_max > cap and whole) else cap
        c = np.where(on, counts[j], 1 << 40)
        best_cnt = int(c.min())
        best_d = (BAND31 - 1) - int(np.argmin(c[::-1]))
        if best_cnt > cap:
            if not qual and best_cnt <= cap_x and narrow(-P * best_cnt, best_d):
                cls[j] = narrow(-P * best_cnt, best_d)
                continue
            if not qual and P > 0 and whole and ge < 0 and go <= ge and not algo & ALN_NO_GAP_CHANCE:
                flag[j] = 4
            continue
        U = -P * best_cnt
        if qual:
            if U <= 3 * G - P:
                continue
            cand = on & (P * counts[j] <= pmax * best_cnt)
            wsum = np.where(cand, weights[j], 1 << 40)
            U = -int(wsum.min())
            best_d = (BAND31 - 1) - int(np.argmin(wsum[::-1]))
        if U > G:
            flag[j] = 0
            continue
        if G - P < U and 2 * G < U and whole and not algo & ALN_NO_SECOND_CHANCE and 1 <= span(go, U) <= 4:
            flag[j] = 3
            continue
        gmax0, gmax1 = span(go, U), span(go - P, U)
        beyond = gmax0 > 4 or gmax1 > 4 or go - 2 * P >= U or 2 * go + ge >= U or 2 * go - P >= U or 3 * go >= U or ge < go
        if whole and not beyond and gmax0 >= 1 and (gmax1 >= 1 or 2 * go >= U):
            flag[j] = 2
            continue
        if not qual and whole:
            cls[j] = narrow(U, best_d)
    return flag, cls


def e2e31_possible_flags(sv, has_quals, M, max_read_len=None):
    """the flag values (and, as 10 + class, the classes) the rule can produce under a scheme at all for reads of M symbols: e2e31_first_pass() on
    whole windows whose centre diagonal holds 0..M mismatches and every other diagonal M (under a ramp each at the smallest penalty)"""
    cnt = np.full((M + 1, BAND31), M, dtype=np.int64)
    cnt[:, 15] = np.arange(M + 1)
    flag, cls = e2e31_first_pass(sv, has_quals, np.full(M + 1, M), np.full(M + 1, M + 31), cnt, weights=cnt * sv[1], max_read_len=max_read_len)
    return {int(f) for f in flag} | {10 + int(c) for c in cls if c}


def e2e31_layout(orc, J, idx=None, with_q=False, read_bits=4):
    """the jobs (all, or `idx`) of e2e31_sweep_jobs() as one packed batch: dict(reads, reads4 -- what the oracle's batch call takes --, bits, roffs,
    quals, text, wb, we, n, max_len, idx)"""
    idx = np.arange(len(J["pats"])) if idx is None else np.asarray(idx)
    S = limit_select(J, idx)
    L = range_layout(S["pats"], S["txts"], S["quals"] if with_q else None)
    return dict(reads=orc.pack4(L["reads"]) if read_bits == 4 else orc.pack2(L["reads"]), reads4=orc.pack4(L["reads"]), bits=read_bits, roffs=L["roffs"],
                quals=L["quals"], text=orc.pack2(L["text"]), wb=L["wb"], we=L["we"], n=len(idx), max_len=int(S["M"].max()), idx=idx)
