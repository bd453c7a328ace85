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
    or 'i32' -- the host's rules (packed_ok() and the binary16 condition of launch_pk_kernel(), csrc/gotoh_banded.hip) restated"""
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
    """packed_ok( SEMI_GLOBAL, ... ) of csrc/gotoh_banded.hip: what the narrow route asks of the band-31 kernel it borrows"""
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
