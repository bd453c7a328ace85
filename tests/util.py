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
