"""nvbio-gpl_amd -- MI355X-native seed-and-extend core behind NVBIO's operator API.

The product is the shared library ``lib/libnvbio_amd.so`` (hand-written HIP kernels for gfx950
behind the C ABI of ``include/nvbio_amd.h``).  This package is the thin host-side mirror of the
reference's interface for the path, for Python callers (tests, bench): the same names and
argument meaning as the reference's C++ templates --

    FMIndex                      nvbio::fm_index / io::FMIndexDataDevice   (nvbio/fmindex/fmindex.h:320-557)
    FMIndexFilter                nvbio::FMIndexFilter<device_tag,...>      (nvbio/fmindex/filter.h:52-231)
    MEMFilter                    nvbio::MEMFilter<device_tag,...>          (nvbio/fmindex/mem.h, mem_inl.h:1303-1528)
    QGramIndex, QGramSetIndex    nvbio::QGramIndexDevice / QGramSetIndexDevice (nvbio/qgram/qgram.h, qgram_inl.h)
    QGroupIndex, QGroupSetIndex  nvbio::QGroupIndexDevice (nvbio/qgram/qgroup.h, qgroup_inl.h) and its set form
    QGramFilter, generate_qgrams nvbio::QGramFilter<device_tag,...>        (nvbio/qgram/filter.h, filter_inl.h)
    set_suffix_sort, set_bwt, suffix_sort, bwt  cuda::suffix_sort / cuda::bwt of string sets and strings (nvbio/sufsort/sufsort.h)
    SimpleGotohScheme, GotohAligner, BestSink semantics                    (nvbio/alignment/utils.h:103-123, alignment.h:437-449)
    BatchedBandedAlignmentScore, batch_banded_alignment_score              (nvbio/alignment/batched.h:104-298)

The ctypes signatures are not written here: ``lib()`` reads them from the header (``abi.bind``; ``pipeline._host_lib()`` does the same with
``include/nvbio_amd_host.h``), so a call site passes plain Python values and a new entry point needs no declaration on this side.  The
``ctypes.Structure`` mirrors of the headers' structs are written by hand and registered in ``_MIRRORS`` at the end of this file; a CPU test
holds each to its header struct, and names every struct without a mirror.

PyTorch is used only as plumbing for device memory and streams.  There is NO CPU fallback:
importing works anywhere (so that symbol checks can run), but every compute entry point raises
``NvbioError`` when the library or a gfx950 device is missing.  Nothing here imports ``oracle``.

The directory name contains a hyphen, so load it with ``__graft_entry__.load_package()``.
"""
import ctypes
import os

import numpy as np

from .abi import bind

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libnvbio_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nvbio_amd.h")
HOST_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nvbio_amd_host.h")      # of lib/libnvbio_amd_host.so (pipeline._host_lib)

GLOBAL, LOCAL, SEMI_GLOBAL = 0, 1, 2
SCORE_MIN = -(1 << 30)
FM_SCAN_FORWARD, FM_COMPLEMENT, FM_NO_KMER_TABLE, FM_NO_VERIFY, FM_COUNT_SECTORS, FM_NO_PIPELINE, FM_DEFER_HEAVY = 1, 2, 4, 8, 16, 32, 64
FM_TABLE_NO_DIRECT, FM_TABLE_NO_CONTEXT, FM_TABLE_NO_GROUPS, FM_TABLE_CANONICAL, FM_TABLE_CANONICAL_WIDE = 1, 2, 4, 8, 16      # nvbio_fm_build_options::table_flags
FM_TABLE_NO_TEXT_PLANES = 32
FM_TABLE_NO_SEED_LOCUS = 64
FM_NO_SEED_LOCUS, FM_COUNT_LOCUS = 128, 4096           # nvbio_fm_match_seed_diagonals_both: the pass without the locus path / its route counts
FM_NO_FAST_RESOLVE, FM_COUNT_RESOLVE = 8192, 16384     # the same pass: every tile resolved by the general code / tiles per path in counts[10:12]
READ_REVERSE, READ_COMPLEMENT = 1, 2
MAX_SEED_OFFSET = 1024            # NVBIO_MAX_SEED_OFFSET: read_len - seed_len at most, for every call that forms diagonal keys
TRACEBACK_SINKS_GIVEN = 1
# nvbio_alignment_batch::algo_flags (which exact shortcuts / kernel variants a call may use; results do not depend on them)
ALN_NO_UNGAPPED_SCORE, ALN_NO_THIRD_CHANCE, ALN_NO_PACKED_DP, ALN_FORCE_PACKED_DP, ALN_NO_UNGAPPED_TRACEBACK, ALN_PK_THREE_WAVES = 1, 2, 4, 8, 16, 32
ALN_NO_NARROW_TRACEBACK, ALN_NO_SECOND_CHANCE, ALN_PK_STRIPE8, ALN_NO_NARROW_SCORE, ALN_NO_BAND_ROUTE = 64, 128, 256, 512, 1024
ALN_NO_QUALITY_SHORTCUT, ALN_RAGGED_READS, ALN_NO_LENGTH_SORT, ALN_NO_F16_DP, ALN_NO_COOPERATIVE_DP, ALN_NO_GAP_CHANCE = 2048, 4096, 8192, 16384, 32768, 65536
ALN_SPLIT_CHANCES, ALN_NO_PAIRED_GAP_CHANCE = 131072, 262144
ALN_NO_NARROW_DP = 524288
ALN_NO_TEXT_PLANES = 1048576
SEED_NO_LOCUS = 2097152           # not an alignment flag: in SeedExtendParams.algo_flags it makes pipeline.seed_pass_begin pass FM_NO_SEED_LOCUS (A/B)
SEED_NO_FAST_RESOLVE = 4194304    # likewise: pipeline.seed_pass_begin passes FM_NO_FAST_RESOLVE (A/B of the common tile's resolution)
ROUTE_SETTLED, ROUTE_FULL_BAND, ROUTE_CLASS_A, ROUTE_CLASS_B, ROUTE_REDONE = 0, 1, 2, 3, 8
DEFAULT_ALGO_FLAGS = 0          # what an AlignmentBatch is created with unless told otherwise (tests set it for a whole run)
BACKTRACK_REFERENCE_QUIRKS = 1

_STATUS = {0: "OK", 1: "INVALID", 2: "HIP", 3: "NOMEM", 4: "UNSUPPORTED", 5: "NO_DEVICE"}


class NvbioError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("nvbio_amd: %s: %s" % (_STATUS.get(status, status), msg))
        self.status = status


# ---- C structs ---------------------------------------------------------------------------------
class _View(ctypes.Structure):
    _fields_ = [("length", ctypes.c_uint32), ("primary", ctypes.c_uint32), ("L2", ctypes.c_uint32 * 5),
                ("bwt_occ_dev", ctypes.c_void_p), ("bwt_occ_words", ctypes.c_uint64),
                ("ssa_dev", ctypes.c_void_p), ("ssa_words", ctypes.c_uint64), ("sa_int", ctypes.c_uint32)]


class _BuildOptions(ctypes.Structure):
    _fields_ = [("kmer_len", ctypes.c_uint32), ("sa_int", ctypes.c_uint32), ("max_lcp", ctypes.c_uint32),
                ("verify", ctypes.c_uint32), ("table_flags", ctypes.c_uint32), ("bucket_symbols", ctypes.c_uint32)]


class _StringSet(ctypes.Structure):
    _fields_ = [("symbols_dev", ctypes.c_void_p), ("symbol_bits", ctypes.c_uint32),
                ("offsets_dev", ctypes.c_void_p), ("offsets_are_ranges", ctypes.c_uint32),
                ("fixed_len", ctypes.c_uint32), ("stride", ctypes.c_uint32), ("n", ctypes.c_uint32),
                ("seeds_per_string", ctypes.c_uint32), ("seed_interval", ctypes.c_uint32),
                ("seed_intervals_dev", ctypes.c_void_p)]


class _Scheme(ctypes.Structure):
    _fields_ = [("match", ctypes.c_int32), ("mm_min", ctypes.c_int32), ("mm_max", ctypes.c_int32),
                ("pat_gap_open", ctypes.c_int32), ("pat_gap_ext", ctypes.c_int32),
                ("txt_gap_open", ctypes.c_int32), ("txt_gap_ext", ctypes.c_int32)]


class _SWScheme(ctypes.Structure):
    _fields_ = [("match", ctypes.c_int32), ("mismatch", ctypes.c_int32), ("deletion", ctypes.c_int32),
                ("insertion", ctypes.c_int32)]


class _Batch(ctypes.Structure):
    _fields_ = [("reads_dev", ctypes.c_void_p), ("read_bits", ctypes.c_uint32),
                ("read_offsets_dev", ctypes.c_void_p), ("quals_dev", ctypes.c_void_p),
                ("read_id_dev", ctypes.c_void_p), ("flags_dev", ctypes.c_void_p),
                ("text_dev", ctypes.c_void_p), ("text_bits", ctypes.c_uint32),
                ("win_begin_dev", ctypes.c_void_p), ("win_end_dev", ctypes.c_void_p), ("n", ctypes.c_uint32),
                ("max_read_len", ctypes.c_uint32), ("algo_flags", ctypes.c_uint32),
                ("text_planes_dev", ctypes.c_void_p)]


class _HitQueues(ctypes.Structure):
    _fields_ = [("idx_queue_dev", ctypes.c_void_p), ("hit_read_id_dev", ctypes.c_void_p), ("hit_seed_dev", ctypes.c_void_p),
                ("hit_loc_dev", ctypes.c_void_p), ("hit_score_dev", ctypes.c_void_p), ("hit_sink_dev", ctypes.c_void_p),
                ("n", ctypes.c_uint32)]


class _SeedHitsParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("seeds_per_read", "first_offset", "seed_interval", "seed_len", "read_len", "max_hits",
                                                "rep_seeds", "max_effort", "min_ext", "max_ext")]


class _RaggedSeedLayout(ctypes.Structure):
    _fields_ = [("read_offsets_dev", ctypes.c_void_p), ("seed_intervals_dev", ctypes.c_void_p)] + \
               [(n, ctypes.c_uint32) for n in ("seeds_per_read", "seeding_pass", "max_reseed", "seed_len", "min_read_len")]


class _RankDict(ctypes.Structure):
    _fields_ = [("text_dev", ctypes.c_void_p), ("word_bits", ctypes.c_uint32), ("occ_dev", ctypes.c_void_p), ("index_bits", ctypes.c_uint32),
                ("K", ctypes.c_uint32), ("length", ctypes.c_uint64)]


_lib = None


def lib():
    """the C-ABI library; raises (loudly) if it has not been built"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NvbioError(5, "%s is missing: build it with __graft_entry__.build() "
                                "(there is no CPU fallback)" % LIB_PATH)
        # torch first: it ships its own HIP runtime, and the library must bind to the one that owns the tensors it is handed
        # (loaded the other way round the two runtimes do not see each other's device context: NVBIO_ERR_NO_DEVICE)
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        bind(L, HEADER_PATH, _MIRRORS)
        _lib = L
    return _lib


def release_scratch():
    """nvbio_amd_release_scratch: give the library's idle scratch blocks back to the driver (it keeps them per stream between calls)"""
    _check(lib().nvbio_amd_release_scratch())


def set_scratch_check(enable, fill_byte=0):
    """nvbio_amd_set_scratch_check: a test tool.  Enabled, every scratch block is a fresh exact-size allocation between two guard
    bands, its layout leaves a gap around each sub-array, and all of it (a caller's temp included) is filled with `fill_byte` before
    any work; enabling clears the report.  Switch it only between calls; query *_temp_bytes after switching."""
    _check(lib().nvbio_amd_set_scratch_check(1 if enable else 0, fill_byte))


def scratch_check_report():
    """nvbio_amd_scratch_check_report, parsed: {tag: (blocks checked, blocks damaged, first bad sub-array, first bad offset)}, the
    last two None for a clean site"""
    buf = ctypes.create_string_buffer(1 << 16)
    _check(lib().nvbio_amd_scratch_check_report(buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        tag, checked, damaged, sub, off = line.split()
        out[tag] = (int(checked), int(damaged), None if sub == "-" else int(sub), None if off == "-" else int(off))
    return out


def _check(status):
    if status != 0:
        raise NvbioError(status, lib().nvbio_amd_last_error().decode())


def _torch():
    import torch
    return torch


_SCRATCH = {}


def _scratch(device, nbytes, cap=8 << 30):
    """one persistent scratch tensor per device for the DP kernels' boundary columns / direction vectors (at most `cap`
    bytes; the library processes a batch in as many launches as the scratch allows).  Handing the library caller scratch
    keeps multi-GiB allocations out of the call (the library would otherwise take a block of its own scratch cache for them and
    keep it).  All users are ordered on the current stream."""
    torch = _torch()
    nbytes = int(min(max(nbytes, 1 << 20), cap))
    key = str(device)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < nbytes:
        _SCRATCH[key] = None
        t = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream_ptr(device):
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_count():
    n = ctypes.c_int(0)
    _check(lib().nvbio_amd_device_count(ctypes.byref(n)))
    return n.value


def _dev_tensor(a, dtype, device):
    """numpy array or tensor -> contiguous device tensor of the given torch dtype (bit pattern kept)"""
    torch = _torch()
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        t = a
        if t.dtype != dtype:
            t = t.view(dtype) if t.element_size() == torch.empty(0, dtype=dtype).element_size() else t.to(dtype)
        return t.to(device).contiguous()
    a = np.ascontiguousarray(a)
    np_of = {torch.int32: np.int32, torch.uint8: np.uint8, torch.int64: np.int64}[dtype]
    if a.dtype.itemsize == np.dtype(np_of).itemsize:
        a = a.view(np_of)
    else:
        a = a.astype(np_of)
    return torch.from_numpy(a).to(device)


# ---- string sets -------------------------------------------------------------------------------
class PackedStringSet:
    """A set of strings in HBM (the string-set concept of FMIndexFilter::rank, filter.h:52-231).

    symbols : packed big-endian uint32 words (bits 2 or 4) or bytes (bits 8), numpy or tensor
    offsets : None (string i = [i*stride, i*stride+fixed_len)), n start offsets (+ fixed_len),
              or n+1 offsets with ranges=True (io::SequenceData sequence_index)
    """

    def __init__(self, symbols, bits, n, offsets=None, ranges=False, fixed_len=0, stride=None, device="cuda:0",
                 seeds_per_string=0, seed_interval=0, seed_intervals=None):
        torch = _torch()
        self.bits, self.n = int(bits), int(n)
        self.symbols = _dev_tensor(symbols, torch.uint8 if bits == 8 else torch.int32, device)
        self.offsets = _dev_tensor(offsets, torch.int32, device)
        self.ranges, self.fixed_len = bool(ranges), int(fixed_len)
        self.stride = int(fixed_len if stride is None else stride)
        self.device = device
        # seed enumeration: n = n_strings * seeds_per_string queries [base(r) + j*seed_interval, + fixed_len)
        self.seeds_per_string, self.seed_interval = int(seeds_per_string), int(seed_interval)
        # ragged seed sets: one seed interval per string (int32 [n_strings]); offsets then hold n_strings + 1 entries and
        # seeds_per_string is the largest seed count of a string (the stride of seed ids)
        self.seed_intervals = _dev_tensor(seed_intervals, torch.int32, device)

    def c_struct(self):
        return _StringSet(_ptr(self.symbols), self.bits, _ptr(self.offsets), 1 if self.ranges else 0,
                          self.fixed_len, self.stride, self.n, self.seeds_per_string, self.seed_interval, _ptr(self.seed_intervals))


# ---- FM-index ----------------------------------------------------------------------------------
class FMIndex:
    """nvbio::fm_index over the production bwt_occ / ssa layout, resident in HBM."""

    def __init__(self, handle, device, keep=()):
        self._h, self.device, self._keep = handle, device, keep
        self._text_src = None                        # (data_ptr, length) of the text build() was given: what text_planes() describe
        self._text_planes = None                     # text_planes() of a built handle, asked once: constant while the handle lives

    @staticmethod
    def _dev_index(device):
        torch = _torch()
        d = torch.device(device)
        return d.index if d.index is not None else 0

    @classmethod
    def from_arrays(cls, length, primary, L2, bwt_occ, ssa, kmer_len=0, sa_int=16, device="cuda:0"):
        """wrap index arrays (numpy or tensors); replaces FMIndexDataDevice (fmindex_impl.cu:740-816)"""
        torch = _torch()
        b = _dev_tensor(bwt_occ, torch.int32, device)
        s = _dev_tensor(ssa, torch.int32, device) if ssa is not None else None
        v = _View()
        v.length, v.primary = int(length), int(primary)
        for i in range(5):
            v.L2[i] = int(L2[i])
        v.bwt_occ_dev, v.bwt_occ_words = b.data_ptr(), b.numel()
        v.ssa_dev, v.ssa_words = (s.data_ptr(), s.numel()) if s is not None else (None, 0)
        v.sa_int = sa_int
        h = ctypes.c_void_p()
        _check(lib().nvbio_fm_index_create(ctypes.byref(v), cls._dev_index(device), kmer_len, _stream_ptr(device), ctypes.byref(h)))
        return cls(h, device, keep=(b, s))

    @classmethod
    def build(cls, text2, length, kmer_len=0, max_lcp=0, sa_int=16, verify=False, device="cuda:0", table_flags=0,
              bucket_symbols=None):
        """build the index on the GPU from a 2-bit packed text (nvbio_fm_index_build).
        table_flags: FM_TABLE_* (which form of the k-mer tables a direct-capable handle keeps; results do not depend on it);
        bucket_symbols: None = automatic, 0..4 forces that many prefix symbols in the suffix sort's bucketing (tests)"""
        torch = _torch()
        t = _dev_tensor(text2, torch.int32, device)
        h = ctypes.c_void_p()
        opts = _BuildOptions(kmer_len, sa_int, max_lcp, 1 if verify else 0, int(table_flags),
                             0 if bucket_symbols is None else 1 + int(bucket_symbols))
        _check(lib().nvbio_fm_index_build(_ptr(t), length, cls._dev_index(device), ctypes.byref(opts), _stream_ptr(device), ctypes.byref(h)))
        fmi = cls(h, device, keep=(t,))
        fmi._text_src = (t.data_ptr(), int(length))
        fmi._text_planes = fmi.text_planes()
        return fmi

    @classmethod
    def load(cls, bwt_path, sa_path=None, kmer_len=0, device="cuda:0"):
        """load the reference's .bwt / .sa files (io::FMIndexDataHost::load, fmindex_impl.cu:333-...)"""
        h = ctypes.c_void_p()
        _check(lib().nvbio_fm_index_load(bwt_path.encode(), sa_path.encode() if sa_path else None, cls._dev_index(device), kmer_len,
                                         _stream_ptr(device), ctypes.byref(h)))
        return cls(h, device)

    def save(self, bwt_path, sa_path=None):
        """write the index in the reference's .bwt / .sa formats (the role of nvBWT)"""
        _check(lib().nvbio_fm_index_save(self._h, bwt_path.encode(), sa_path.encode() if sa_path else None,
                                         _stream_ptr(self.device)))

    def close(self):
        if self._h is not None:
            _torch().cuda.synchronize(self.device)
            _check(lib().nvbio_fm_index_destroy(self._h))
            self._h = None
            self._seed_bufs = None                   # the pipeline's per-strand seed-pass buffers (pipeline.seed_and_extend)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def view(self):
        v = _View()
        _check(lib().nvbio_fm_index_get_view(self._h, ctypes.byref(v)))
        return v

    @property
    def length(self):
        return self.view().length

    @property
    def primary(self):
        return self.view().primary

    def arrays(self):
        """(bwt_occ, ssa) copied out into fresh device int32 tensors (nvbio_fm_index_export)"""
        torch = _torch()
        v = self.view()
        b = torch.empty(int(v.bwt_occ_words), dtype=torch.int32, device=self.device)
        s = torch.empty(int(v.ssa_words), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_index_export(self._h, _ptr(b), _ptr(s), _stream_ptr(self.device)))
        return b, s

    def device_bytes(self):
        b = ctypes.c_uint64()
        _check(lib().nvbio_fm_index_device_bytes(self._h, ctypes.byref(b)))
        return b.value

    def text_planes(self):
        """nvbio_fm_index_text_planes: (device pointer, length) of the text as bit planes -- what AlignmentBatch(text_planes=) takes, valid
        while the handle lives -- or None for a handle without them (no text kept, or built with FM_TABLE_NO_TEXT_PLANES)"""
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        _check(lib().nvbio_fm_index_text_planes(self._h, ctypes.byref(p), ctypes.byref(n)))
        return (p.value, n.value) if p.value else None

    def seed_locus(self):
        """nvbio_fm_index_seed_locus: (device pointer, seed length) of the seed locus lines the handle keeps -- what lets the two-strand seed
        pass settle a read's other seeds once its first seed has placed it -- or None for a handle without them"""
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        _check(lib().nvbio_fm_index_seed_locus(self._h, ctypes.byref(p), ctypes.byref(n)))
        return (p.value, n.value) if p.value else None

    def build_seed_locus(self, seed_len, out=None):
        """out is None: nvbio_fm_index_build_seed_locus -- the handle builds its own lines, or rebuilds them for another seed length
        (kmer_len .. kmer_len + 7; no seed pass of the handle may be in flight).  out: a 128-byte aligned uint8 tensor of
        seed_locus_bytes(length) bytes -- nvbio_seed_locus_build fills it instead and the handle's own lines stay as they are; returns out"""
        if out is None:
            _check(lib().nvbio_fm_index_build_seed_locus(self._h, seed_len, _stream_ptr(self.device)))
            return None
        _check(lib().nvbio_seed_locus_build(self._h, seed_len, _ptr(out), _stream_ptr(self.device)))
        return out

    def text_planes_of(self, text2, length):
        """text_planes()'s pointer if the handle was built from this very text -- the same device address and length -- else None
        (no call into the library: build() asked once)"""
        tp = self._text_planes if self._h is not None else None
        same = tp is not None and self._text_src == (text2.data_ptr(), int(length)) and tp[1] == int(length)
        return tp[0] if same else None

    # -- free functions of nvbio/fmindex/fmindex.h:370-557 ---------------------------------------
    def match(self, queries, flags=0, want_blocks=False):
        """ranges[n,2] (int32 tensor holding uint32 bits) = match()/match_reverse() of every query"""
        torch = _torch()
        ranges = torch.empty((queries.n, 2), dtype=torch.int32, device=self.device)
        blocks = torch.empty(queries.n, dtype=torch.int32, device=self.device) if want_blocks else None
        qs = queries.c_struct()
        _check(lib().nvbio_fm_match(self._h, ctypes.byref(qs), flags, _ptr(ranges), _ptr(blocks), _stream_ptr(self.device)))
        return (ranges, blocks) if want_blocks else ranges

    def supports_direct(self):
        yes = ctypes.c_int(0)
        _check(lib().nvbio_fm_index_supports_direct(self._h, ctypes.byref(yes)))
        return bool(yes.value)

    def match_direct(self, queries, flags=0):
        """(ranges, direct): as match(), but searches that collapse to one SA row finish on the text and report
        the occurrence's text position, flagged in direct (nvbio_fm_match_direct; needs an index built with sa_int=1)"""
        torch = _torch()
        ranges = torch.empty((queries.n, 2), dtype=torch.int32, device=self.device)
        direct = torch.empty(queries.n, dtype=torch.uint8, device=self.device)
        qs = queries.c_struct()
        _check(lib().nvbio_fm_match_direct(self._h, ctypes.byref(qs), flags, _ptr(ranges), _ptr(direct), _stream_ptr(self.device)))
        return ranges, direct

    def hamming_backtrack(self, queries, seed_len, mismatches, quirks=False, max_ranges=0):
        """nvbio::hamming_backtrack with a counting delegate (nvbio_fm_hamming_backtrack) -> (counts, n_ranges, ranges or None)"""
        torch = _torch()
        counts = torch.empty(queries.n, dtype=torch.int32, device=self.device)
        nr = torch.empty(queries.n, dtype=torch.int32, device=self.device)
        rg = torch.zeros((queries.n, max_ranges, 2), dtype=torch.int32, device=self.device) if max_ranges else None
        qs = queries.c_struct()
        _check(lib().nvbio_fm_hamming_backtrack(self._h, ctypes.byref(qs), seed_len, mismatches, BACKTRACK_REFERENCE_QUIRKS if quirks else 0,
                                                _ptr(counts), _ptr(nr), _ptr(rg), max_ranges, _stream_ptr(self.device)))
        return counts, nr, rg

    def match_seed_diagonals(self, seeds, flags, read_len, strand, buffers=None, grid_blocks=0):
        """the seed pass of one strand straight to candidate diagonals (nvbio_fm_match_seed_diagonals) -> the buffers dict:
        "keys" int64 (the first counts[0] are valid, in seed order), "ranges" int32 [., 2] and "ids" int32 (the first counts[1]:
        the residual seeds on several SA rows), "counts" int32 [2] (on the device: the caller reads them).
        buffers: optional dict reused across calls (the output arrays and the call's scratch);
        grid_blocks: cap of the launch in workgroups, a multiple of 64 (0 = the library's choice; results do not depend on it)"""
        torch = _torch()
        n = seeds.n
        if buffers is None:
            buffers = {}
        qs = seeds.c_struct()
        if buffers.get("n") != n or buffers.get("spr") != seeds.seeds_per_string:
            buffers["n"], buffers["spr"] = n, seeds.seeds_per_string
            # keys: only as many as there can be candidates are ever written; sized for the worst case like the residual arrays
            buffers["keys"] = torch.empty(n, dtype=torch.int64, device=self.device)
            buffers["ranges"] = torch.empty((n, 2), dtype=torch.int32, device=self.device)
            buffers["ids"] = torch.empty(n, dtype=torch.int32, device=self.device)
            buffers["counts"] = torch.empty(4, dtype=torch.int32, device=self.device)     # [2:4]: FM_COUNT_SECTORS' uint64
            nb = ctypes.c_uint64(0)
            _check(lib().nvbio_fm_match_seed_diagonals_temp_bytes(ctypes.byref(qs), ctypes.byref(nb)))
            buffers["temp"] = torch.empty(nb.value, dtype=torch.uint8, device=self.device)
        assert grid_blocks % 64 == 0 and grid_blocks < (1 << 22)
        _check(lib().nvbio_fm_match_seed_diagonals(self._h, ctypes.byref(qs), flags | ((grid_blocks // 64) << 16), read_len, strand,
                                                   _ptr(buffers["keys"]), _ptr(buffers["ranges"]), _ptr(buffers["ids"]), _ptr(buffers["counts"]),
                                                   _ptr(buffers["temp"]), buffers["temp"].numel(), _stream_ptr(self.device)))
        return buffers

    @property
    def canonical_kmer(self):
        """k of the canonical two-strand table the handle holds (built with FM_TABLE_CANONICAL; seeds of k .. k + 7 symbols), 0 if none"""
        return lib().nvbio_fm_index_is_canonical(self._h)

    @property
    def canonical(self):
        return self.canonical_kmer != 0

    def match_seed_diagonals_both(self, seeds, read_len, buffers=None, flags=0, grid_blocks=0, inline_hits=0, defer_heavy=False):
        """the seed pass of BOTH strands in one launch over the canonical table (nvbio_fm_match_seed_diagonals_both) -> the buffers dict:
        "keys" int64 (the first counts[0]: both strands, tile by tile), "ranges" int32 [2 n, 2] / "ids" int32 [2 n]: residual seeds on
        several rows, forward strand in [0, counts[1]), reverse strand in [n, n + counts[2]); "counts" int32 [12] on the device
        ([4:6]: FM_COUNT_SECTORS' uint64, [6:10]: FM_COUNT_LOCUS' route counts, [10:12]: FM_COUNT_RESOLVE's tiles per path).
        flags: FM_NO_SEED_LOCUS runs the pass without the locus path (seed_locus(): same results either way); FM_NO_FAST_RESOLVE
        resolves every tile by the general code (same results either way; the common way exists with 4-bit reads, 16-byte entries and
        defer_heavy only, and FM_COUNT_RESOLVE accounts for the launch of the same flags: pass defer_heavy with it).
        inline_hits (2..4): a search that ends on up to that many rows leaves all their keys in "keys" instead of a residual entry.
        "tile_offsets" int32 [n_tiles + 1]: tile t (the reads [t * reads_per_tile, (t + 1) * reads_per_tile)) owns keys[tile_offsets[t] :
        tile_offsets[t + 1]]; counts[3] = tile_offsets[n_tiles], the keys in tile order (deferred searches append theirs behind them)."""
        torch = _torch()
        n = seeds.n
        if buffers is None:
            buffers = {}
        qs = seeds.c_struct()
        if buffers.get("n") != n or buffers.get("spr") != seeds.seeds_per_string:
            buffers["n"], buffers["spr"] = n, seeds.seeds_per_string
            cap = ctypes.c_uint64(0)
            _check(lib().nvbio_fm_match_seed_diagonals_both_keys_capacity(ctypes.byref(qs), ctypes.byref(cap)))
            buffers["keys"] = torch.empty(max(int(cap.value), 1), dtype=torch.int64, device=self.device)
            buffers["ranges"] = torch.empty((2 * n, 2), dtype=torch.int32, device=self.device)
            buffers["ids"] = torch.empty(2 * n, dtype=torch.int32, device=self.device)
            buffers["counts"] = torch.zeros(12, dtype=torch.int32, device=self.device)    # [4:6]: FM_COUNT_SECTORS' uint64, [6:10]: FM_COUNT_LOCUS, [10:12]: FM_COUNT_RESOLVE
            nb = ctypes.c_uint64(0)
            _check(lib().nvbio_fm_match_seed_diagonals_both_temp_bytes(ctypes.byref(qs), ctypes.byref(nb)))
            buffers["temp"] = torch.empty(nb.value, dtype=torch.uint8, device=self.device)
            rpt, nt = ctypes.c_uint32(0), ctypes.c_uint32(0)
            _check(lib().nvbio_fm_seed_tiles(ctypes.byref(qs), ctypes.byref(rpt), ctypes.byref(nt)))
            buffers["reads_per_tile"], buffers["n_tiles"] = int(rpt.value), int(nt.value)
            buffers["tile_offsets"] = torch.zeros(int(nt.value) + 1, dtype=torch.int32, device=self.device)
        assert grid_blocks % 64 == 0 and grid_blocks < (1 << 22)
        _check(lib().nvbio_fm_match_seed_diagonals_both_tiled(
            self._h, ctypes.byref(qs), flags | (FM_DEFER_HEAVY if defer_heavy else 0) | ((int(inline_hits) & 15) << 8) | ((grid_blocks // 64) << 16),
            read_len, _ptr(buffers["keys"]), _ptr(buffers["ranges"]), _ptr(buffers["ids"]), n, _ptr(buffers["counts"]), _ptr(buffers["tile_offsets"]),
            _ptr(buffers["temp"]), buffers["temp"].numel(), _stream_ptr(self.device)))
        return buffers

    def residual_diagonals(self, ranges, ids, cap, seeds_per_read, seed_interval, seed_len, read_len, read_offsets=None, seed_intervals=None):
        """nvbio_fm_residual_diagonals: the first `cap` rows of every residual range located and turned into diagonal keys (duplicates of
        neighbouring seeds dropped) -> (keys int64 [n * cap], n_keys int32 [1] on the device)"""
        torch = _torch()
        n = int(ids.numel())
        keys = torch.empty(max(n * int(cap), 1), dtype=torch.int64, device=self.device)
        n_keys = torch.zeros(1, dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_residual_diagonals(
            self._h, _ptr(ranges), _ptr(ids), n, int(cap), seeds_per_read, seed_interval, seed_len, read_len, _ptr(read_offsets),
            _ptr(seed_intervals), _ptr(keys), _ptr(n_keys), _stream_ptr(self.device)))
        return keys, n_keys

    def rank(self, rows, syms):
        torch = _torch()
        rows = _dev_tensor(rows, torch.int32, self.device)
        syms = _dev_tensor(syms, torch.uint8, self.device)
        out = torch.empty(rows.numel(), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_rank(self._h, _ptr(rows), _ptr(syms), rows.numel(), _ptr(out), _stream_ptr(self.device)))
        return out

    def rank4(self, rows):
        torch = _torch()
        rows = _dev_tensor(rows, torch.int32, self.device)
        out = torch.empty((rows.numel(), 4), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_rank4(self._h, _ptr(rows), rows.numel(), _ptr(out), _stream_ptr(self.device)))
        return out

    def basic_inv_psi(self, rows):
        torch = _torch()
        rows = _dev_tensor(rows, torch.int32, self.device)
        out = torch.empty(rows.numel(), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_basic_inv_psi(self._h, _ptr(rows), rows.numel(), _ptr(out), _stream_ptr(self.device)))
        return out

    def locate(self, rows):
        torch = _torch()
        rows = _dev_tensor(rows, torch.int32, self.device)
        pos = torch.empty(rows.numel(), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_locate(self._h, _ptr(rows), rows.numel(), _ptr(pos), _stream_ptr(self.device)))
        return pos

    def locate_ssa_iterator(self, rows):
        torch = _torch()
        rows = _dev_tensor(rows, torch.int32, self.device)
        jt = torch.empty((rows.numel(), 2), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_locate_init(self._h, _ptr(rows), rows.numel(), _ptr(jt), _stream_ptr(self.device)))
        return jt

    def lookup_ssa_iterator(self, jt):
        torch = _torch()
        pos = torch.empty(jt.shape[0], dtype=torch.int32, device=self.device)
        _check(lib().nvbio_fm_locate_lookup(self._h, _ptr(jt), jt.shape[0], _ptr(pos), _stream_ptr(self.device)))
        return pos


class FMIndexFilter:
    """nvbio::FMIndexFilter<device_tag, fm_index_type> (nvbio/fmindex/filter.h:136-231)."""

    def __init__(self):
        self._index = None
        self._ranges = self._slots = self._direct = None
        self._n_hits = 0
        self._n_queries = 0

    def rank(self, index, string_set, flags=0):
        """enact the filter; returns the total number of hits (filter_inl.h:261-293)"""
        torch = _torch()
        self._index, self._n_queries, self._direct = index, string_set.n, None
        self._ranges = torch.empty((string_set.n, 2), dtype=torch.int32, device=index.device)
        self._slots = torch.empty(string_set.n, dtype=torch.int64, device=index.device)
        total = ctypes.c_uint64(0)
        qs = string_set.c_struct()
        _check(lib().nvbio_fm_filter_rank(index._h, ctypes.byref(qs), flags, _ptr(self._ranges), _ptr(self._slots), ctypes.byref(total),
                                          _stream_ptr(index.device)))
        self._n_hits = total.value
        return self._n_hits

    def rank_ranges(self, index, ranges, direct=None):
        """the scan half of rank() over ranges already computed by FMIndex.match (nvbio_fm_filter_scan), or by
        FMIndex.match_direct (then pass its `direct` flags: locate() copies the positions those ranges hold)"""
        torch = _torch()
        self._index, self._n_queries, self._ranges, self._direct = index, ranges.shape[0], ranges, direct
        self._slots = torch.empty(ranges.shape[0], dtype=torch.int64, device=index.device)
        total = ctypes.c_uint64(0)
        _check(lib().nvbio_fm_filter_scan(index._h, _ptr(ranges), ranges.shape[0], _ptr(self._slots), ctypes.byref(total), _stream_ptr(index.device)))
        self._n_hits = total.value
        return self._n_hits

    def locate(self, begin, end, hits=None):
        """hits[h-begin] = (text_pos, query_id) for hit indices [begin,end) (filter_inl.h:299-393)"""
        torch = _torch()
        if hits is None:
            hits = torch.empty((end - begin, 2), dtype=torch.int32, device=self._index.device)
        if self._direct is not None:
            _check(lib().nvbio_fm_filter_locate_direct(self._index._h, _ptr(self._ranges), _ptr(self._slots), _ptr(self._direct), self._n_queries,
                                                       begin, end, _ptr(hits), _stream_ptr(self._index.device)))
            return hits
        _check(lib().nvbio_fm_filter_locate(self._index._h, _ptr(self._ranges), _ptr(self._slots), self._n_queries, begin, end, _ptr(hits),
                                            _stream_ptr(self._index.device)))
        return hits

    def locate_diagonals(self, begin, end, seeds_per_read, seed_interval, seed_len, read_len, strand, query_ids=None, read_offsets=None,
                         seed_intervals=None):
        """locate() and hits_to_diagonals() in one pass (nvbio_fm_filter_locate_diagonals): int64 keys
        read << 34 | strand << 33 | diagonal + 1024 of hit indices [begin, end); query_ids: the seed id of every range when
        the ranges are a compacted subset (FMIndex.match_seed_diagonals' residual list)"""
        torch = _torch()
        keys = torch.empty(end - begin, dtype=torch.int64, device=self._index.device)
        if read_offsets is not None:                 # ragged reads: every read's length and seed interval
            _check(lib().nvbio_fm_filter_locate_diagonals_ragged(
                self._index._h, _ptr(self._ranges), _ptr(self._slots), _ptr(self._direct), self._n_queries, begin, end, seeds_per_read, seed_len,
                _ptr(read_offsets), _ptr(seed_intervals), strand, _ptr(query_ids), _ptr(keys), _stream_ptr(self._index.device)))
            return keys
        _check(lib().nvbio_fm_filter_locate_diagonals(
            self._index._h, _ptr(self._ranges), _ptr(self._slots), _ptr(self._direct), self._n_queries, begin, end, seeds_per_read, seed_interval,
            seed_len, read_len, strand, _ptr(query_ids), _ptr(keys), _stream_ptr(self._index.device)))
        return keys

    def n_hits(self):
        return self._n_hits

    def ranges(self):
        return self._ranges

    def slots(self):
        return self._slots


class _MemParams(ctypes.Structure):
    _fields_ = [("min_intv", ctypes.c_uint32), ("max_intv", ctypes.c_uint32), ("min_span", ctypes.c_uint32),
                ("split_len", ctypes.c_uint32), ("split_width", ctypes.c_uint32)]


MEM_GROUP_FLAG = 1 << 31
MEM_UNLIMITED = 0xFFFFFFFF


class MEMFilter:
    """nvbio::MEMFilter<device_tag, fm_index_type> (nvbio/fmindex/mem.h:270-360): the maximal exact matches of every read over a
    forward index and the index of the reversed text (nvbio_mem_filter_*; the departures from the reference are listed in
    include/nvbio_amd.h)."""

    def __init__(self):
        self._index = None
        self._ranges = self._slots = self._first = self._temp = None
        self._n_ranges = self._n_mems = self._n_queries = 0
        self.records = 0                             # bwt_occ records the last rank() gathered
        self.attempts = 0                            # library calls the last rank() made (1 unless a buffer had to grow)

    @staticmethod
    def _symbols(string_set):
        """the symbols of a plain string set: a bound on its MEM ranges without split (a read has at most one range per symbol)"""
        n = string_set.n
        if n and string_set.offsets is not None and string_set.ranges:
            ends = string_set.offsets[[0, n]].cpu().numpy().astype(np.uint32).astype(np.int64)
            return int(ends[1] - ends[0])
        return n * string_set.fixed_len

    def rank(self, f_index, r_index, string_set, min_intv=1, max_intv=MEM_UNLIMITED, min_span=1, split_len=MEM_UNLIMITED,
             split_width=MEM_UNLIMITED, max_ranges=None):
        """enact the filter; returns the total number of MEM occurrences (mem_inl.h:1303-1445).
        max_ranges None: the range buffers hold the reads' symbol total (a bound without split) or what an earlier call needed,
        whichever is larger, and grow when a split call needs more -- a call that has to grow repeats every pass, so a filter
        reused over batches pays that at most once.  An explicit max_ranges that is too small raises NvbioError naming the
        number needed (so does a temp that is too small)."""
        torch = _torch()
        dev = f_index.device
        params = _MemParams(min_intv, max_intv, min_span, split_len, split_width)
        qs = string_set.c_struct()
        tb = ctypes.c_uint64(0)
        _check(lib().nvbio_mem_filter_temp_bytes(ctypes.byref(qs), ctypes.byref(params), ctypes.byref(tb), _stream_ptr(dev)))
        n = string_set.n
        self._index, self._n_queries = f_index, n
        self._first = torch.empty(n + 1, dtype=torch.int32, device=dev)
        if max_ranges is None:
            held = 0 if self._ranges is None or self._ranges.device != torch.device(dev) else self._ranges.shape[0]
            cap = max(1, held, self._symbols(string_set))
        else:
            cap = max(1, int(max_ranges))
        if self._ranges is None or self._ranges.shape[0] != cap or self._ranges.device != torch.device(dev):
            self._ranges = torch.empty((cap, 4), dtype=torch.int32, device=dev)
            self._slots = torch.empty(cap, dtype=torch.int64, device=dev)
        if self._temp is None or self._temp.numel() < tb.value or self._temp.device != torch.device(dev):
            self._temp = torch.empty(max(int(tb.value), 1), dtype=torch.uint8, device=dev)
        self.attempts = 0
        while True:
            nr, nm, rec = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            self.attempts += 1
            st = lib().nvbio_mem_filter_rank(f_index._h, r_index._h, ctypes.byref(qs), ctypes.byref(params), _ptr(self._ranges), cap,
                                             _ptr(self._first), _ptr(self._slots), _ptr(self._temp), self._temp.numel(), ctypes.byref(nr),
                                             ctypes.byref(nm), ctypes.byref(rec), _stream_ptr(dev))
            if st == 1 and max_ranges is None:
                msg = lib().nvbio_amd_last_error().decode()
                if "max_ranges" in msg and nr.value > cap:
                    cap = nr.value
                    self._ranges = torch.empty((cap, 4), dtype=torch.int32, device=dev)
                    self._slots = torch.empty(cap, dtype=torch.int64, device=dev)
                    continue
                if "temp_bytes" in msg:
                    import re
                    need = int(re.search(r"needs (\d+)", msg).group(1))
                    if need > self._temp.numel():
                        self._temp = None
                        self._temp = torch.empty(need, dtype=torch.uint8, device=dev)
                        continue
            _check(st)
            break
        self._n_ranges, self._n_mems, self.records = nr.value, nm.value, rec.value
        return self._n_mems

    @property
    def n_ranges(self):
        return self._n_ranges

    def n_mems(self):
        return self._n_mems

    def ranges(self):
        """[n_ranges, 4] int32 (uint32 bits): SA x, SA y, string id | MEM_GROUP_FLAG, span begin | span end << 16"""
        return self._ranges[:self._n_ranges]

    def slots(self):
        return self._slots[:self._n_ranges]

    def first_ranges(self):
        """[n_strings + 1]: the index of every string's first range"""
        return self._first

    def first_hit(self, string_id):
        """index of the first MEM occurrence of string_id (mem_inl.h:1449-1461); n_mems past the last string"""
        if string_id >= self._n_queries:
            return self._n_mems
        r = int(self._first[string_id].item())
        return int(self._slots[r - 1].item()) if r else 0

    def locate(self, begin, end, hits=None):
        """hits[h - begin] = (text position, string id, span begin, span end) for MEM occurrences [begin, end) (mem_inl.h:1463-1505)"""
        torch = _torch()
        if hits is None:
            hits = torch.empty((max(end - begin, 0), 4), dtype=torch.int32, device=self._index.device)
        if end > begin:
            _check(lib().nvbio_mem_filter_locate(self._index._h, _ptr(self._ranges), _ptr(self._slots), self._n_ranges, begin, end, _ptr(hits),
                                                 _stream_ptr(self._index.device)))
        return hits


# ---- q-gram seeding -----------------------------------------------------------------------------
class _QGramView(ctypes.Structure):
    _fields_ = [("q", ctypes.c_uint32), ("symbol_size", ctypes.c_uint32), ("qlut", ctypes.c_uint32), ("is_set", ctypes.c_uint32),
                ("n_qgrams", ctypes.c_uint32), ("n_unique", ctypes.c_uint32), ("lut_size", ctypes.c_uint64), ("device", ctypes.c_int),
                ("qgrams_dev", ctypes.c_void_p), ("slots_dev", ctypes.c_void_p), ("index_dev", ctypes.c_void_p), ("lut_dev", ctypes.c_void_p)]


def _qgram_text(text, bits, device):
    torch = _torch()
    return _dev_tensor(text, torch.uint8 if bits == 8 else torch.int32, device)


class QGramIndex:
    """nvbio::QGramIndexDevice (nvbio/qgram/qgram.h, qgram_inl.h:30-140): the q-grams of every position of a text (nvbio_qgram_*; the
    packing, ordering and departures are listed in include/nvbio_amd.h).  The arrays are views of the handle's device memory."""
    IS_SET = False

    def __init__(self, handle, device, keep=()):
        self._h, self.device, self._keep = handle, device, keep

    @classmethod
    def build(cls, text, text_bits, length, q, symbol_size=2, qlut=0, device="cuda:0"):
        """QGramIndexDevice::build( q, symbol_size, length, text, qlut ); text: packed words (bits 2, 4) or bytes (8)"""
        t = _qgram_text(text, text_bits, device)
        h = ctypes.c_void_p()
        _check(lib().nvbio_qgram_index_build(FMIndex._dev_index(device), _ptr(t), text_bits, length, q, symbol_size, qlut, ctypes.byref(h),
                                             _stream_ptr(device)))
        return cls(h, device)

    def close(self):
        if getattr(self, "_h", None):
            lib().nvbio_qgram_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def view(self):
        v = _QGramView()
        _check(lib().nvbio_qgram_index_get_view(self._h, ctypes.byref(v)))
        return v

    def device_bytes(self):
        b = ctypes.c_uint64(0)
        _check(lib().nvbio_qgram_index_device_bytes(self._h, ctypes.byref(b)))
        return b.value

    def arrays(self):
        """copies of the index arrays as device tensors (nvbio_qgram_index_export): qgrams int64 [n_unique], slots int32
        [n_unique + 1], index int32 [n_qgrams] (or [n_qgrams, 2] (string_id, string_pos) for a set index), lut int32
        [lut_size + 1] or None (uint bit patterns)"""
        torch = _torch()
        v = self.view()
        qg = torch.empty(max(v.n_unique, 1), dtype=torch.int64, device=self.device)
        sl = torch.empty(v.n_unique + 1, dtype=torch.int32, device=self.device)
        ix = torch.empty((max(v.n_qgrams, 1), 2) if v.is_set else max(v.n_qgrams, 1), dtype=torch.int32, device=self.device)
        lut = torch.empty(v.lut_size + 1, dtype=torch.int32, device=self.device) if v.lut_dev else None
        _check(lib().nvbio_qgram_index_export(self._h, _ptr(qg), _ptr(sl), _ptr(ix), _ptr(lut), _stream_ptr(self.device)))
        return dict(qgrams=qg[:v.n_unique], slots=sl, index=ix[:v.n_qgrams], lut=lut)

    @property
    def q(self):
        return self.view().q

    @property
    def n_qgrams(self):
        return self.view().n_qgrams

    @property
    def n_unique(self):
        return self.view().n_unique

    def ranges(self, qgrams):
        """the index as a search functor: int32 [n, 2] half-open (begin, end) slots of each q-gram, (0, 0) on a miss"""
        torch = _torch()
        g = _dev_tensor(qgrams, torch.int64, self.device)
        out = torch.empty((g.numel(), 2), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_qgram_ranges(self._h, _ptr(g), g.numel(), _ptr(out), _stream_ptr(self.device)))
        return out


class QGramSetIndex(QGramIndex):
    """nvbio::QGramSetIndexDevice (qgram_inl.h:186-300): the q-grams of the seeds k * seed_interval of every string of a plain set"""
    IS_SET = True

    @classmethod
    def build(cls, string_set, q, symbol_size=2, seed_interval=1, qlut=0):
        """QGramSetIndexDevice::build( q, symbol_size, string_set, uniform_seeds_functor( q, seed_interval ), qlut )"""
        h = ctypes.c_void_p()
        ss = string_set.c_struct()
        dev = string_set.device
        _check(lib().nvbio_qgram_set_index_build(FMIndex._dev_index(dev), ctypes.byref(ss), q, symbol_size, seed_interval, qlut, ctypes.byref(h),
                                                 _stream_ptr(dev)))
        return cls(h, dev, keep=(string_set,))


class _QGroupView(ctypes.Structure):
    _fields_ = [("q", ctypes.c_uint32), ("symbol_size", ctypes.c_uint32), ("is_set", ctypes.c_uint32), ("n_qgrams", ctypes.c_uint32),
                ("n_unique", ctypes.c_uint32), ("n_words", ctypes.c_uint64), ("device", ctypes.c_int), ("table_dev", ctypes.c_void_p),
                ("ss_dev", ctypes.c_void_p), ("p_dev", ctypes.c_void_p)]


class QGroupIndex(QGramIndex):
    """nvbio::QGroupIndexDevice (nvbio/qgram/qgroup.h, qgroup_inl.h:162-277): the q-group index of every position of a text, the
    O(1)-lookup alternative to QGramIndex (nvbio_qgroup_*; the structure, layout and departures are listed in include/nvbio_amd.h).
    Usable wherever QGramFilter.rank takes an index; ranges(), q, n_qgrams, n_unique, device_bytes() and close() are inherited."""

    @classmethod
    def build(cls, text, text_bits, length, q, symbol_size=2, device="cuda:0"):
        """QGroupIndexDevice::build( q, symbol_size, length, text ); text: packed words (bits 2, 4) or bytes (8)"""
        t = _qgram_text(text, text_bits, device)
        h = ctypes.c_void_p()
        _check(lib().nvbio_qgroup_index_build(FMIndex._dev_index(device), _ptr(t), text_bits, length, q, symbol_size, ctypes.byref(h),
                                              _stream_ptr(device)))
        return cls(h, device)

    def view(self):
        v = _QGroupView()
        _check(lib().nvbio_qgroup_index_get_view(self._h, ctypes.byref(v)))
        return v

    def arrays(self):
        """copies of the index arrays as device tensors (nvbio_qgroup_index_export), in the reference's layout: I int32 [n_words],
        S int32 [n_words], SS int32 [n_unique + 1], P int32 [n_qgrams] (or [n_qgrams, 2] (string_id, string_pos) for a set index)
        (uint bit patterns)"""
        torch = _torch()
        v = self.view()
        I = torch.empty(v.n_words, dtype=torch.int32, device=self.device)
        S = torch.empty(v.n_words, dtype=torch.int32, device=self.device)
        SS = torch.empty(v.n_unique + 1, dtype=torch.int32, device=self.device)
        P = torch.empty((max(v.n_qgrams, 1), 2) if v.is_set else max(v.n_qgrams, 1), dtype=torch.int32, device=self.device)
        _check(lib().nvbio_qgroup_index_export(self._h, _ptr(I), _ptr(S), _ptr(SS), _ptr(P), _stream_ptr(self.device)))
        return dict(I=I, S=S, SS=SS, P=P[:v.n_qgrams])


class QGroupSetIndex(QGroupIndex):
    """the q-group index of the seeds k * seed_interval of every string of a plain set, seeded as QGramSetIndex (the reference has
    no set form; PEANUT indexes the reads)"""
    IS_SET = True

    @classmethod
    def build(cls, string_set, q, symbol_size=2, seed_interval=1):
        h = ctypes.c_void_p()
        ss = string_set.c_struct()
        dev = string_set.device
        _check(lib().nvbio_qgroup_set_index_build(FMIndex._dev_index(dev), ctypes.byref(ss), q, symbol_size, seed_interval, ctypes.byref(h),
                                                  _stream_ptr(dev)))
        return cls(h, dev, keep=(string_set,))


# ---- sufsort -------------------------------------------------------------------------------------
SUFSORT_NO_EMPTY_SUFFIXES = 1


class _SufsortStats(ctypes.Structure):
    _fields_ = [("n_suffixes", ctypes.c_uint32), ("rounds", ctypes.c_uint32), ("sorted_per_round", ctypes.c_uint32 * 16),
                ("symbols_per_word", ctypes.c_uint32), ("peak_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return dict(n_suffixes=self.n_suffixes, rounds=self.rounds, sorted_per_round=list(self.sorted_per_round),
                    symbols_per_word=self.symbols_per_word, peak_bytes=self.peak_bytes)


def set_suffix_count(string_set, flags=0):
    """nvbio_set_suffix_count: the suffixes set_suffix_sort / set_bwt write: sum( len + 1 ), or sum( len ) with
    SUFSORT_NO_EMPTY_SUFFIXES"""
    n = ctypes.c_uint32(0)
    ss = string_set.c_struct()
    dev = string_set.device
    _check(lib().nvbio_set_suffix_count(FMIndex._dev_index(dev), ctypes.byref(ss), flags, ctypes.byref(n), _stream_ptr(dev)))
    return n.value


def set_suffix_sort(string_set, flags=0, want_global=True, capacity=None):
    """cuda::suffix_sort( string_set ) (nvbio/sufsort/sufsort.h; nvbio_set_suffix_sort): (suffixes int32 [n, 2] = (pos, string_id) in
    sorted order, global int32 [n] = the reference's global suffix indices or None, stats dict); uint bit patterns.  The order is
    stated in include/nvbio_amd.h.  capacity: the entries to allocate (default: the count)"""
    torch = _torch()
    dev = string_set.device
    cap = set_suffix_count(string_set, flags) if capacity is None else int(capacity)
    suf = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)
    glb = torch.empty(max(cap, 1), dtype=torch.int32, device=dev) if want_global else None
    n, st = ctypes.c_uint32(0), _SufsortStats()
    ss = string_set.c_struct()
    _check(lib().nvbio_set_suffix_sort(FMIndex._dev_index(dev), ctypes.byref(ss), flags, _ptr(suf), _ptr(glb), cap, ctypes.byref(n), ctypes.byref(st),
                                       _stream_ptr(dev)))
    return suf[:n.value], (glb[:n.value] if want_global else None), st.as_dict()


def set_suffix_sort_flat(string_set, flags=0):
    """the sort in the form the reference's suffix handler takes (nvbio_set_suffix_sort_flat): (suffix_array int32 [n] = global suffix
    indices in sorted order, string_ids int32 [n], cum_lengths int32 [N] = the inclusive scan of the strings' suffix counts, stats)"""
    torch = _torch()
    dev = string_set.device
    cap = set_suffix_count(string_set, flags)
    sa = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    ids = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    cum = torch.empty(max(string_set.n, 1), dtype=torch.int32, device=dev)
    n, st = ctypes.c_uint32(0), _SufsortStats()
    ss = string_set.c_struct()
    _check(lib().nvbio_set_suffix_sort_flat(FMIndex._dev_index(dev), ctypes.byref(ss), flags, _ptr(sa), _ptr(ids), _ptr(cum), cap, ctypes.byref(n),
                                            ctypes.byref(st), _stream_ptr(dev)))
    return sa[:n.value], ids[:n.value], cum[:string_set.n], st.as_dict()


def set_bwt(string_set, flags=0, want_suffixes=True, capacity=None):
    """cuda::bwt( string_set ) (the engine of nvSetBWT; nvbio_set_bwt): (bwt uint8 [n], the symbol in front of each sorted suffix, 255
    in front of a string; suffixes int32 [n, 2] or None; stats dict)"""
    torch = _torch()
    dev = string_set.device
    cap = set_suffix_count(string_set, flags) if capacity is None else int(capacity)
    bwt = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    suf = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev) if want_suffixes else None
    n, st = ctypes.c_uint32(0), _SufsortStats()
    ss = string_set.c_struct()
    _check(lib().nvbio_set_bwt(FMIndex._dev_index(dev), ctypes.byref(ss), flags, _ptr(bwt), _ptr(suf), cap, ctypes.byref(n), ctypes.byref(st),
                               _stream_ptr(dev)))
    return bwt[:n.value], (suf[:n.value] if want_suffixes else None), st.as_dict()


def suffix_sort(text2, length, device="cuda:0"):
    """cuda::suffix_sort( string ) (nvbio_suffix_sort): the suffix array int32 [length + 1] of a 2-bit packed text, row 0 = the empty
    suffix (nvbio/fmindex/bwt.h:28-37); uint bit patterns"""
    torch = _torch()
    t = _dev_tensor(text2, torch.int32, device)
    sa = torch.empty(int(length) + 1, dtype=torch.int32, device=device)
    _check(lib().nvbio_suffix_sort(_ptr(t), length, FMIndex._dev_index(device), _ptr(sa), _stream_ptr(device)))
    return sa


def bwt(text2, length, device="cuda:0"):
    """cuda::bwt( string ) with find_primary (nvbio_bwt): (bwt words int32 [ceil( length / 16 )], 2-bit big-endian packed with the
    primary row squeezed out, as nvbio_fm_index_build interleaves them; primary)"""
    torch = _torch()
    t = _dev_tensor(text2, torch.int32, device)
    words = torch.empty((int(length) + 15) // 16, dtype=torch.int32, device=device)
    primary = ctypes.c_uint32(0)
    _check(lib().nvbio_bwt(_ptr(t), length, FMIndex._dev_index(device), _ptr(words), ctypes.byref(primary), _stream_ptr(device)))
    return words, primary.value


_GENERATE_TEMP = {}


def generate_qgrams(q, symbol_size, text, text_bits, text_len, first_pos, n, sort=False, device="cuda:0"):
    """qmap's build_qgrams (examples/qmap/qmap.cu:75-99, nvbio_generate_qgrams): (qgrams int64 [n], positions int32 [n]) of text
    positions [first_pos, first_pos + n), padded past text_len; sort: the pairs stably sorted by q-gram"""
    torch = _torch()
    t = _qgram_text(text, text_bits, device)
    qg = torch.empty(n, dtype=torch.int64, device=device)
    ix = torch.empty(n, dtype=torch.int32, device=device)
    tb = ctypes.c_uint64(0)
    _check(lib().nvbio_generate_qgrams_temp_bytes(n, 1 if sort else 0, ctypes.byref(tb)))
    key = str(device)
    temp = _GENERATE_TEMP.get(key)
    if tb.value and (temp is None or temp.numel() < tb.value):
        _GENERATE_TEMP[key] = None
        temp = _GENERATE_TEMP[key] = torch.empty(int(tb.value), dtype=torch.uint8, device=device)
    _check(lib().nvbio_generate_qgrams(FMIndex._dev_index(device), q, symbol_size, _ptr(t), text_bits, text_len, first_pos, n, _ptr(qg), _ptr(ix),
                                       1 if sort else 0, _ptr(temp) if tb.value else None, temp.numel() if tb.value else 0, _stream_ptr(device)))
    return qg, ix


class QGramFilter:
    """nvbio::QGramFilter<device_tag, qgram_index_type, ...> (nvbio/qgram/filter.h, filter_inl.h:336-483).  Owns its ranges, slots,
    hits, merge outputs and temp, and keeps their sizes across batches."""

    def __init__(self):
        self._index = None
        self._ranges = self._slots = self._indices = self._temp = None
        self._merged = self._counts = None
        self._n_queries = self._n_hits = 0

    def _grow_temp(self, nbytes, dev):
        torch = _torch()
        if self._temp is None or self._temp.numel() < nbytes or self._temp.device != torch.device(dev):
            self._temp = None
            self._temp = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)

    def rank(self, index, qgrams, indices):
        """enact the filter over the query q-grams (int64) and their coordinates (int32, e.g. text positions); returns the number of
        hits (filter_inl.h:336-380)"""
        torch = _torch()
        dev = index.device
        g = _dev_tensor(qgrams, torch.int64, dev)
        ix = _dev_tensor(indices, torch.int32, dev)
        n = g.numel()
        self._index, self._n_queries, self._indices = index, n, ix
        if self._ranges is None or self._ranges.shape[0] < n or self._ranges.device != torch.device(dev):
            self._ranges = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
            self._slots = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        tb = ctypes.c_uint64(0)
        _check(lib().nvbio_qgram_filter_temp_bytes(n, ctypes.byref(tb)))
        self._grow_temp(tb.value, dev)
        nh = ctypes.c_uint64(0)
        _check(lib().nvbio_qgram_filter_rank(index._h, _ptr(g), n, _ptr(self._ranges), _ptr(self._slots), _ptr(self._temp), self._temp.numel(),
                                             ctypes.byref(nh), _stream_ptr(dev)))
        self._n_hits = nh.value
        return self._n_hits

    def n_hits(self):
        return self._n_hits

    def ranges(self):
        """int32 [n_queries, 2]: the half-open slots of every query q-gram"""
        return self._ranges[:self._n_queries]

    def slots(self):
        """int64 [n_queries]: the inclusive scan of the range sizes"""
        return self._slots[:self._n_queries]

    def locate(self, begin, end, hits=None):
        """hits of outputs [begin, end): int32 [end - begin, 2] (index position, query coordinate) for a string index,
        [end - begin, 4] (string_id, string_pos, query coordinate, 0) for a set index (filter_inl.h:386-410)"""
        torch = _torch()
        cols = 4 if self._index.IS_SET else 2
        if hits is None:
            hits = torch.empty((max(end - begin, 0), cols), dtype=torch.int32, device=self._index.device)
        if end > begin:
            _check(lib().nvbio_qgram_filter_locate(self._index._h, _ptr(self._ranges), _ptr(self._slots), _ptr(self._indices), self._n_queries, begin,
                                                   end, _ptr(hits), _stream_ptr(self._index.device)))
        return hits

    def merge(self, interval, hits, is_set=None):
        """merge hits by snapped diagonal (filter_inl.h:446-483): (merged, counts) -- int32 [n_merged] diagonals for string hits or
        [n_merged, 2] (diagonal, string_id) for set hits, and int32 [n_merged] counts (uint32 bit patterns)"""
        torch = _torch()
        if is_set is None:
            is_set = hits.dim() == 2 and hits.shape[1] == 4
        dev = hits.device
        n = hits.shape[0]
        tb = ctypes.c_uint64(0)
        _check(lib().nvbio_qgram_filter_merge_temp_bytes(1 if is_set else 0, n, ctypes.byref(tb)))
        self._grow_temp(tb.value, dev)
        if self._merged is None or self._merged.shape[0] < max(n, 1) or self._merged.device != dev:
            self._merged = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
            self._counts = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        nm = ctypes.c_uint32(0)
        hits = hits.contiguous()
        _check(lib().nvbio_qgram_filter_merge(FMIndex._dev_index(dev), 1 if is_set else 0, interval, _ptr(hits), n, _ptr(self._merged),
                                              _ptr(self._counts), ctypes.byref(nm), _ptr(self._temp), self._temp.numel(), _stream_ptr(dev)))
        m = nm.value
        merged = self._merged.view(-1)[:2 * m].view(m, 2) if is_set else self._merged.view(-1)[:m]
        return merged.clone(), self._counts[:m].clone()


# ---- alignment ---------------------------------------------------------------------------------
class GotohScheme:
    """the Gotoh scoring-scheme concept as data (see nvbio_gotoh_scheme in include/nvbio_amd.h)"""

    def __init__(self, match, mm_min, mm_max, pat_gap_open, pat_gap_ext, txt_gap_open, txt_gap_ext):
        self.c = _Scheme(match, mm_min, mm_max, pat_gap_open, pat_gap_ext, txt_gap_open, txt_gap_ext)


def SimpleGotohScheme(match, mismatch, gap_open, gap_ext):
    """aln::SimpleGotohScheme (nvbio/alignment/utils.h:103-123)"""
    return GotohScheme(match, -mismatch, -mismatch, gap_open, gap_ext, gap_open, gap_ext)


def EditDistanceScheme():
    """the scheme under which the Gotoh kernels compute the reference's edit-distance aligner: EditDistanceSWScheme
    (match 0, mismatch -1, insertion = deletion = -1; nvbio/alignment/ed/ed_banded_inl.h:37-69 runs the banded
    linear-gap SW with it), and with open = extension the affine recurrences give the same H in every cell -- pinned
    against the reference in tests/golden/ed_golden.npz"""
    return GotohScheme(0, 1, 1, -1, -1, -1, -1)


class SimpleSmithWatermanScheme:
    """aln::SimpleSmithWatermanScheme(match, mismatch, deletion, insertion) (nvbio/alignment/utils.h:81-98), signed scores"""

    def __init__(self, match, mismatch, deletion, insertion):
        self.c = _SWScheme(match, mismatch, deletion, insertion)


class SmithWatermanAligner:
    """aln::SmithWatermanAligner<TYPE, scheme> (nvbio/alignment/alignment.h:508-545): linear gaps.  `.sw` is what the
    scoring entry points take (nvbio_banded_sw_score / nvbio_full_sw_score); `.scheme` is the Gotoh form with open =
    extension, which exists when deletion == insertion and is what the banded traceback takes."""

    def __init__(self, type, scheme):
        self.type, self.sw = type, scheme
        c = scheme.c
        self.scheme = (GotohScheme(c.match, -c.mismatch, -c.mismatch, c.deletion, c.deletion, c.deletion, c.deletion)
                       if c.deletion == c.insertion else None)


def make_smith_waterman_aligner(type, scheme):
    """aln::make_smith_waterman_aligner<TYPE>(scheme) (nvbio/alignment/alignment.h:529)"""
    return SmithWatermanAligner(type, scheme)


def make_edit_distance_aligner(type):
    """aln::make_edit_distance_aligner<TYPE>() (nvbio/alignment/alignment.h:382): the Smith-Waterman aligner with
    EditDistanceSWScheme (0, -1, -1, -1) (ed/ed_utils.h:36-43) -- the aligner of examples/fmmap/fmmap.cu:346-359 and of
    nvBowtie --scoring ed (banded), and the full-matrix one of ed/ed_inl.h"""
    return SmithWatermanAligner(type, SimpleSmithWatermanScheme(0, -1, -1, -1))


class GotohAligner:
    """aln::GotohAligner<TYPE, scheme> (nvbio/alignment/alignment.h:437-449)"""

    def __init__(self, type, scheme):
        self.type, self.scheme = type, scheme


def make_gotoh_aligner(type, scheme):
    return GotohAligner(type, scheme)


class AlignmentBatch:
    """The flattened stream of alignment jobs (see nvbio_alignment_batch)."""

    def __init__(self, reads, read_bits, read_offsets, text, text_bits, win_begin, win_end, quals=None, read_id=None,
                 flags=None, device="cuda:0", max_read_len=0, algo_flags=None, text_planes=None):
        """text_planes: the text as bit planes -- a device pointer (FMIndex.text_planes()[0], FMIndex.text_planes_of) or a uint8 tensor
        filled by build_text_planes -- of THIS text as it stands, or None"""
        torch = _torch()
        self.device = device
        self.text_planes = text_planes
        self.algo_flags = DEFAULT_ALGO_FLAGS if algo_flags is None else int(algo_flags)
        self.read_bits, self.text_bits = int(read_bits), int(text_bits)
        self.reads = _dev_tensor(reads, torch.uint8 if read_bits == 8 else torch.int32, device)
        self.read_offsets = _dev_tensor(read_offsets, torch.int32, device)
        self.text = _dev_tensor(text, torch.uint8 if text_bits == 8 else torch.int32, device)
        self.win_begin = _dev_tensor(win_begin, torch.int32, device)
        self.win_end = _dev_tensor(win_end, torch.int32, device)
        self.quals = _dev_tensor(quals, torch.uint8, device)
        self.read_id = _dev_tensor(read_id, torch.int32, device)
        self.flags = _dev_tensor(flags, torch.uint8, device)
        self.n = int(self.win_begin.numel())
        self.max_read_len = int(max_read_len)       # max_pattern_length() of the stream concept; 0 = unknown

    def size(self):
        return self.n

    def c_struct(self):
        return _Batch(_ptr(self.reads), self.read_bits, _ptr(self.read_offsets), _ptr(self.quals), _ptr(self.read_id),
                      _ptr(self.flags), _ptr(self.text), self.text_bits, _ptr(self.win_begin), _ptr(self.win_end),
                      self.n, self.max_read_len, self.algo_flags,
                      ctypes.c_void_p(self.text_planes.data_ptr() if hasattr(self.text_planes, "data_ptr") else self.text_planes))


def seed_locus_bytes(length):
    """nvbio_seed_locus_bytes: the size of the seed locus lines of a text (FMIndex.build_seed_locus(out=))"""
    b = ctypes.c_uint64()
    _check(lib().nvbio_seed_locus_bytes(length, ctypes.byref(b)))
    return b.value


def text_planes_bytes(length):
    b = ctypes.c_uint64()
    _check(lib().nvbio_text_planes_bytes(length, ctypes.byref(b)))
    return b.value


def build_text_planes(text2, length, device="cuda:0", out=None):
    """nvbio_text_planes_build: the 2-bit packed text as bit planes (include/nvbio_amd.h: the layout), a uint8 tensor of
    text_planes_bytes(length) bytes; `out`: the caller's buffer (128-byte aligned) instead of a fresh one"""
    torch = _torch()
    t = _dev_tensor(text2, torch.int32, device)
    if out is None:
        out = torch.empty(text_planes_bytes(length), dtype=torch.uint8, device=device)
    _check(lib().nvbio_text_planes_build(FMIndex._dev_index(device), _ptr(t), length, _ptr(out), _stream_ptr(device)))
    return out


DEVICE_THREAD_SCHEDULER = "DeviceThreadScheduler"
DEVICE_STAGED_THREAD_SCHEDULER = "DeviceStagedThreadScheduler"     # nvbio/alignment/batched.h: the 32-row-window work queue


class BatchedBandedAlignmentScore:
    """aln::BatchedBandedAlignmentScore<BAND_LEN, stream, scheduler> (nvbio/alignment/batched.h:298,
    batched_banded_inl.h:90-157): enact() scores every job of the stream.  scheduler =
    DEVICE_STAGED_THREAD_SCHEDULER gives the results of the staged specialization (batched_banded_inl.h:165-236): 32-row windows
    with the min_score exit; min_scores (int32 per job, or one int) is then the stream's context->min_score."""

    def __init__(self, band_len, aligner, scheduler=DEVICE_THREAD_SCHEDULER):
        self.band_len, self.aligner, self.scheduler = int(band_len), aligner, scheduler
        if scheduler not in (DEVICE_THREAD_SCHEDULER, DEVICE_STAGED_THREAD_SCHEDULER):
            raise NvbioError(1, "unknown scheduler %r" % (scheduler,))

    def min_temp_storage(self, max_pattern_len, max_text_len, stream_size):
        # as the reference's Host/Device thread schedulers (batched_banded_inl.h:100-104); its staged scheduler asks for one band of
        # short2 checkpoints per queue slot (:176-191) -- this library keeps the band in registers and needs none
        return 0

    max_temp_storage = min_temp_storage

    def enact(self, batch, scores=None, sinks=None, min_scores=None):
        torch = _torch()
        if scores is None:
            scores = torch.empty(batch.n, dtype=torch.int32, device=batch.device)
        if sinks is None:
            sinks = torch.empty((batch.n, 2), dtype=torch.int32, device=batch.device)
        bs = batch.c_struct()
        sw = getattr(self.aligner, "sw", None)
        if self.scheduler == DEVICE_STAGED_THREAD_SCHEDULER:
            if sw is not None:
                raise NvbioError(4, "the staged scheduler is instantiated for Gotoh aligners")
            per_job = min_scores is not None and not isinstance(min_scores, int)
            if per_job and (min_scores.dtype != torch.int32 or min_scores.numel() != batch.n):
                raise NvbioError(1, "min_scores: int32 per job")
            _check(lib().nvbio_banded_gotoh_score_staged(
                FMIndex._dev_index(batch.device), self.band_len, self.aligner.type, ctypes.byref(self.aligner.scheme.c), ctypes.byref(bs),
                _ptr(min_scores) if per_job else None, SCORE_MIN if min_scores is None else (0 if per_job else int(min_scores)), _ptr(scores),
                _ptr(sinks), _stream_ptr(batch.device)))
            return scores, sinks
        fn = lib().nvbio_banded_sw_score if sw is not None else lib().nvbio_banded_gotoh_score
        _check(fn(FMIndex._dev_index(batch.device), self.band_len, self.aligner.type, ctypes.byref(sw.c if sw is not None else self.aligner.scheme.c),
                  ctypes.byref(bs), _ptr(scores), _ptr(sinks), _stream_ptr(batch.device)))
        return scores, sinks


def batch_banded_alignment_score(band_len, aligner, batch):
    """aln::batch_banded_alignment_score<BAND_LEN> (nvbio/alignment/batched.h:185, batched_inl.h:1046-1086)"""
    return BatchedBandedAlignmentScore(band_len, aligner).enact(batch)


def banded_gotoh_score_routes(band_len, aligner, batch):
    """nvbio_banded_gotoh_score_routes: (scores, sinks) as batch_banded_alignment_score plus one uint8 per job, the route it took:
    ROUTE_SETTLED, ROUTE_FULL_BAND, ROUTE_CLASS_A or ROUTE_CLASS_B, + ROUTE_REDONE for a class job the full band had to redo"""
    torch = _torch()
    scores = torch.empty(batch.n, dtype=torch.int32, device=batch.device)
    sinks = torch.empty((batch.n, 2), dtype=torch.int32, device=batch.device)
    routes = torch.empty(batch.n, dtype=torch.uint8, device=batch.device)
    bs = batch.c_struct()
    _check(lib().nvbio_banded_gotoh_score_routes(FMIndex._dev_index(batch.device), int(band_len), aligner.type, ctypes.byref(aligner.scheme.c),
                                                 ctypes.byref(bs), _ptr(scores), _ptr(sinks), _ptr(routes), _stream_ptr(batch.device)))
    return scores, sinks, routes


TB_ROUTE_SETTLED, TB_ROUTE_FULL_BAND, TB_ROUTE_BAND15, TB_ROUTE_BAND7 = 0, 1, 2, 3


def banded_gotoh_traceback_routes(band_len, aligner, batch, cigar_stride=64, temp=None, scores=None, sinks=None):
    """nvbio_banded_gotoh_traceback_routes: (scores, sources, sinks, cigars, lens) as BatchedBandedAlignmentTraceback.enact plus two
    uint8 per job: the route it took (TB_ROUTE_SETTLED -- the ungapped shortcut, or nothing traced --, TB_ROUTE_FULL_BAND,
    TB_ROUTE_BAND15 or TB_ROUTE_BAND7) and, for the two narrow routes, the first column of its band (0 otherwise)"""
    torch = _torch()
    n, dev = batch.n, batch.device
    given = scores is not None and sinks is not None
    if not given:
        scores = torch.empty(n, dtype=torch.int32, device=dev)
        sinks = torch.empty((n, 2), dtype=torch.int32, device=dev)
    sources = torch.empty((n, 2), dtype=torch.int32, device=dev)
    cigars = torch.zeros((n, cigar_stride), dtype=torch.int16, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    routes = torch.empty(n, dtype=torch.uint8, device=dev)
    band_off = torch.empty(n, dtype=torch.uint8, device=dev)
    bs = batch.c_struct()
    _check(lib().nvbio_banded_gotoh_traceback_routes(
        FMIndex._dev_index(dev), int(band_len), aligner.type, ctypes.byref(aligner.scheme.c), ctypes.byref(bs), _ptr(scores), _ptr(sources),
        _ptr(sinks), _ptr(cigars), cigar_stride, _ptr(lens), TRACEBACK_SINKS_GIVEN if given else 0, _ptr(temp),
        0 if temp is None else temp.numel() * temp.element_size(), _ptr(routes), _ptr(band_off), _stream_ptr(dev)))
    return scores, sources, sinks, cigars, lens, routes, band_off


FULL_TB_ROUTE_SETTLED, FULL_TB_ROUTE_ALL_ROWS, FULL_TB_ROUTE_RESTRICTED, FULL_TB_ROUTE_BAND15 = 0, 1, 2, 3


def full_gotoh_traceback_routes(aligner, batch, max_pattern_len, max_text_len, min_scores=None, cigar_stride=64, temp=None, scores=None, sinks=None):
    """nvbio_full_gotoh_traceback_routes: (scores, sources, sinks, cigars, lens) as BatchedAlignmentTraceback.enact plus two uint8 per
    job: the route it took (FULL_TB_ROUTE_SETTLED -- the diagonal through the sink, a skipped job, or nothing traced --,
    FULL_TB_ROUTE_ALL_ROWS, FULL_TB_ROUTE_RESTRICTED or FULL_TB_ROUTE_BAND15) and, for the last two, the gap bound G it ran with (0 otherwise)"""
    torch = _torch()
    n, dev = batch.n, batch.device
    given = scores is not None and sinks is not None
    if not given:
        scores = torch.empty(n, dtype=torch.int32, device=dev)
        sinks = torch.empty((n, 2), dtype=torch.int32, device=dev)
    sources = torch.empty((n, 2), dtype=torch.int32, device=dev)
    cigars = torch.zeros((n, cigar_stride), dtype=torch.int16, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    routes = torch.empty(n, dtype=torch.uint8, device=dev)
    gap_bound = torch.empty(n, dtype=torch.uint8, device=dev)
    ms = _dev_tensor(min_scores, torch.int32, dev)
    bs = batch.c_struct()
    if temp is None and n:
        temp = _scratch(dev, BatchedAlignmentTraceback(aligner).min_temp_storage(batch, max_pattern_len, max_text_len))
    _check(lib().nvbio_full_gotoh_traceback_routes(
        FMIndex._dev_index(dev), aligner.type, ctypes.byref(aligner.scheme.c), ctypes.byref(bs),
        max_pattern_len, max_text_len, _ptr(ms), _ptr(scores), _ptr(sources), _ptr(sinks), _ptr(cigars), cigar_stride, _ptr(lens),
        TRACEBACK_SINKS_GIVEN if given else 0, _ptr(temp), 0 if temp is None else temp.numel() * temp.element_size(),
        _ptr(routes), _ptr(gap_bound), _stream_ptr(dev)))
    return scores, sources, sinks, cigars, lens, routes, gap_bound


GAP_PAIR_MAX_SHIFT = 5
NO_PARTNER = 0xFFFFFFFF


def banded_gap_pairs(batch):
    """nvbio_banded_gap_pairs: for every job of the batch the job the band-31 end-to-end scorer may run it with as ONE gap-chance job
    (uint32 on the device, NO_PARTNER where there is none) -- a function of the batch's geometry alone, see ALN_NO_PAIRED_GAP_CHANCE"""
    torch = _torch()
    partner = torch.empty(batch.n, dtype=torch.int32, device=batch.device)
    bs = batch.c_struct()
    _check(lib().nvbio_banded_gap_pairs(FMIndex._dev_index(batch.device), ctypes.byref(bs), _ptr(partner), _stream_ptr(batch.device)))
    return partner


class BatchedBandedAlignmentTraceback:
    """aln::BatchedBandedAlignmentTraceback<BAND_LEN,CHECKPOINTS,stream> (nvbio/alignment/batched.h,
    batched_banded_inl.h) with nvBowtie's run-length Backtracker (alignment_utils.h:115-157) as the stream's
    backtracer: per job the Alignment {score, source, sink} and its io::Cigar elements in backtracking order"""

    def __init__(self, band_len, aligner):
        self.band_len, self.aligner = int(band_len), aligner

    def min_temp_storage(self, batch):
        out = ctypes.c_uint64(0)
        bs = batch.c_struct()
        _check(lib().nvbio_banded_gotoh_traceback_temp_bytes(ctypes.byref(bs), self.band_len, ctypes.byref(out)))
        return int(out.value)

    def enact(self, batch, cigar_stride=64, temp=None, scores=None, sinks=None):
        """scores / sinks: optional results of BatchedBandedAlignmentScore for the same batch (the scoring pass is
        then skipped, NVBIO_TRACEBACK_SINKS_GIVEN)"""
        torch = _torch()
        n, dev = batch.n, batch.device
        given = scores is not None and sinks is not None
        if not given:
            scores = torch.empty(n, dtype=torch.int32, device=dev)
            sinks = torch.empty((n, 2), dtype=torch.int32, device=dev)
        sources = torch.empty((n, 2), dtype=torch.int32, device=dev)
        cigars = torch.zeros((n, cigar_stride), dtype=torch.int16, device=dev)
        lens = torch.empty(n, dtype=torch.int32, device=dev)
        bs = batch.c_struct()
        sw = getattr(self.aligner, "sw", None)                      # the linear-gap Smith-Waterman / edit-distance aligners
        fn = lib().nvbio_banded_sw_traceback if sw is not None else lib().nvbio_banded_gotoh_traceback
        _check(fn(
            FMIndex._dev_index(dev), self.band_len, self.aligner.type, ctypes.byref(sw.c if sw is not None else self.aligner.scheme.c),
            ctypes.byref(bs), _ptr(scores), _ptr(sources), _ptr(sinks), _ptr(cigars), cigar_stride, _ptr(lens), TRACEBACK_SINKS_GIVEN if given else 0,
            _ptr(temp), 0 if temp is None else temp.numel() * temp.element_size(), _stream_ptr(dev)))
        return scores, sources, sinks, cigars, lens


class BatchedAlignmentTraceback:
    """aln::BatchedAlignmentTraceback<CHECKPOINTS,stream> (full-matrix DP; nvbio/alignment/batched.h:395-411) with
    nvBowtie's run-length Backtracker: Alignment {score, source, sink} (x = text, y = pattern) and io::Cigar runs"""

    def __init__(self, aligner):
        self.aligner = aligner

    def min_temp_storage(self, batch, max_pattern_len, max_text_len):
        out = ctypes.c_uint64(0)
        bs = batch.c_struct()
        _check(lib().nvbio_full_gotoh_traceback_temp_bytes(ctypes.byref(bs), max_pattern_len, max_text_len, ctypes.byref(out)))
        return int(out.value)

    def enact(self, batch, max_pattern_len, max_text_len, min_scores=None, cigar_stride=64, temp=None, scores=None, sinks=None):
        torch = _torch()
        n, dev = batch.n, batch.device
        given = scores is not None and sinks is not None
        if not given:
            scores = torch.empty(n, dtype=torch.int32, device=dev)
            sinks = torch.empty((n, 2), dtype=torch.int32, device=dev)
        sources = torch.empty((n, 2), dtype=torch.int32, device=dev)
        cigars = torch.zeros((n, cigar_stride), dtype=torch.int16, device=dev)
        lens = torch.empty(n, dtype=torch.int32, device=dev)
        ms = _dev_tensor(min_scores, torch.int32, dev)
        bs = batch.c_struct()
        if temp is None and n:
            temp = _scratch(dev, self.min_temp_storage(batch, max_pattern_len, max_text_len))
        sw = getattr(self.aligner, "sw", None)                      # the linear-gap Smith-Waterman / edit-distance aligners
        fn = lib().nvbio_full_sw_traceback if sw is not None else lib().nvbio_full_gotoh_traceback
        _check(fn(
            FMIndex._dev_index(dev), self.aligner.type, ctypes.byref(sw.c if sw is not None else self.aligner.scheme.c), ctypes.byref(bs),
            max_pattern_len, max_text_len, _ptr(ms), _ptr(scores), _ptr(sources), _ptr(sinks), _ptr(cigars), cigar_stride, _ptr(lens),
            TRACEBACK_SINKS_GIVEN if given else 0, _ptr(temp), 0 if temp is None else temp.numel() * temp.element_size(), _stream_ptr(dev)))
        return scores, sources, sinks, cigars, lens


def finish_alignment(batch, sources, cigars, cigar_lens, mds_stride=0):
    """nvBowtie finish_alignment (traceback_inl.h:536-705) on the outputs of a traceback: (ed, mds, mds_lens) --
    edit distance per job and, with mds_stride > 0, the MDS byte streams [n, mds_stride]"""
    torch = _torch()
    n, dev = batch.n, batch.device
    ed = torch.empty(n, dtype=torch.int32, device=dev)
    mds = torch.zeros((n, mds_stride), dtype=torch.uint8, device=dev) if mds_stride else None
    ml = torch.empty(n, dtype=torch.int32, device=dev) if mds_stride else None
    bs = batch.c_struct()
    _check(lib().nvbio_finish_alignment(FMIndex._dev_index(dev), ctypes.byref(bs), _ptr(sources), _ptr(cigars), cigars.shape[1], _ptr(cigar_lens),
                                        _ptr(ed), _ptr(mds), mds_stride, _ptr(ml), _stream_ptr(dev)))
    return ed, mds, ml


def cigar_string(cigar_row, length, forward=True):
    """render one alignment's io::Cigar elements ('3M2D147M'); forward=True reverses the backtracking order"""
    els = [int(c) & 0xFFFF for c in cigar_row[:length]]
    if forward:
        els = els[::-1]
    return "".join("%d%s" % (c >> 2, "MIDS"[c & 3]) for c in els)


class BatchedAlignmentScore:
    """aln::BatchedAlignmentScore<stream, scheduler> (full-matrix DP; batched.h:274, batched_inl.h:221-592)"""

    def __init__(self, aligner, text_blocking=True):
        self.aligner, self.text_blocking = aligner, bool(text_blocking)

    def enact(self, batch, max_pattern_len, max_text_len, min_scores=None, scores=None, sinks=None):
        torch = _torch()
        if scores is None:
            scores = torch.empty(batch.n, dtype=torch.int32, device=batch.device)
        if sinks is None:
            sinks = torch.empty((batch.n, 2), dtype=torch.int32, device=batch.device)
        ms = _dev_tensor(min_scores, torch.int32, batch.device)
        bs = batch.c_struct()
        sw = getattr(self.aligner, "sw", None)
        fn = lib().nvbio_full_sw_score if sw is not None else lib().nvbio_full_gotoh_score
        rows = max_pattern_len if self.text_blocking else max_text_len
        temp = _scratch(batch.device, batch.n * max(rows, 1) * 4)
        _check(fn(FMIndex._dev_index(batch.device), self.aligner.type, 1 if self.text_blocking else 0,
                  ctypes.byref(sw.c if sw is not None else self.aligner.scheme.c), ctypes.byref(bs), max_pattern_len, max_text_len, _ptr(ms),
                  _ptr(scores), _ptr(sinks), _ptr(temp), temp.numel(), _stream_ptr(batch.device)))
        return scores, sinks


def batch_banded_alignment_score_best2(band_len, aligner, batch, distinct_dist=0):
    """banded scoring into aln::Best2Sink<int32>(distinct_dist) (nvbio/alignment/sink.h:96-116)
    -> (scores, sinks, scores2, sinks2)"""
    torch = _torch()
    sc = [torch.empty(batch.n, dtype=torch.int32, device=batch.device) for _ in range(2)]
    sk = [torch.empty((batch.n, 2), dtype=torch.int32, device=batch.device) for _ in range(2)]
    bs = batch.c_struct()
    _check(lib().nvbio_banded_gotoh_score_best2(FMIndex._dev_index(batch.device), band_len, aligner.type, ctypes.byref(aligner.scheme.c),
                                                ctypes.byref(bs), distinct_dist, _ptr(sc[0]), _ptr(sk[0]), _ptr(sc[1]), _ptr(sk[1]),
                                                _stream_ptr(batch.device)))
    return sc[0], sk[0], sc[1], sk[1]


def batch_alignment_score_best2(aligner, batch, max_pattern_len, max_text_len, distinct_dist=0, text_blocking=False, min_scores=None):
    """full-matrix scoring into aln::Best2Sink<int32>(distinct_dist) -> (scores, sinks, scores2, sinks2)"""
    torch = _torch()
    sc = [torch.empty(batch.n, dtype=torch.int32, device=batch.device) for _ in range(2)]
    sk = [torch.empty((batch.n, 2), dtype=torch.int32, device=batch.device) for _ in range(2)]
    ms = _dev_tensor(min_scores, torch.int32, batch.device)
    bs = batch.c_struct()
    _check(lib().nvbio_full_gotoh_score_best2(FMIndex._dev_index(batch.device), aligner.type, 1 if text_blocking else 0,
                                              ctypes.byref(aligner.scheme.c), ctypes.byref(bs), max_pattern_len, max_text_len, _ptr(ms),
                                              distinct_dist, _ptr(sc[0]), _ptr(sk[0]), _ptr(sc[1]), _ptr(sk[1]), _stream_ptr(batch.device)))
    return sc[0], sk[0], sc[1], sk[1]


def hits_to_diagonals(hits, seeds_per_read, seed_interval, seed_len, read_len, strand):
    """hit_to_diagonal (examples/fmmap/fmmap.cu:92-117): int64 keys read<<34 | strand<<33 | diagonal+1024"""
    torch = _torch()
    keys = torch.empty(hits.shape[0], dtype=torch.int64, device=hits.device)
    _check(lib().nvbio_hits_to_diagonals(FMIndex._dev_index(hits.device), _ptr(hits), hits.shape[0], seeds_per_read, seed_interval, seed_len,
                                         read_len, strand, _ptr(keys), _stream_ptr(hits.device)))
    return keys


def best_candidate_reduce(keys, scores, sinks, win_begin, best):
    """best[read] = max(best[read], selection key of each candidate) by 64-bit atomic max (nvbio_best_candidate_reduce);
    best: int64 tensor, zero-initialised by the caller, one entry per read"""
    _check(lib().nvbio_best_candidate_reduce(FMIndex._dev_index(keys.device), _ptr(keys), _ptr(scores), _ptr(sinks), _ptr(win_begin), keys.shape[0],
                                             _ptr(best), _stream_ptr(keys.device)))
    return best


def best_candidate_unpack(best):
    """(score int32, end position int64 or -1, strand uint8) per read from the keys of best_candidate_reduce"""
    torch = _torch()
    n, dev = best.shape[0], best.device
    score = torch.empty(n, dtype=torch.int32, device=dev); pos = torch.empty(n, dtype=torch.int64, device=dev)
    rc = torch.empty(n, dtype=torch.uint8, device=dev)
    _check(lib().nvbio_best_candidate_unpack(FMIndex._dev_index(dev), _ptr(best), n, _ptr(score), _ptr(pos), _ptr(rc), _stream_ptr(dev)))
    return score, pos, rc


def best_candidate_windows(keys, scores, sinks, win_begin, best, best_wb, best_locus=None):
    """nvbio_best_candidate_windows: atomic max of the window begin (and locus) of the candidates that ARE their read's best (`best`:
    the final keys of best_candidate_reduce) into best_wb / best_locus (int64 per read, initialised to -1 by the caller)"""
    if keys.numel() == 0:
        return
    _check(lib().nvbio_best_candidate_windows(FMIndex._dev_index(keys.device), _ptr(keys), _ptr(scores), _ptr(sinks), _ptr(win_begin), keys.numel(),
                                              _ptr(best), _ptr(best_wb), _ptr(best_locus), _stream_ptr(keys.device)))


def traceback_best_batch(best, best_wb, read_len, band, genome_len, min_score, read_offsets=None, min_scores=None):
    """nvbio_traceback_best_batch: the per-read arrays of the traceback batch of every read's best alignment ->
    (flags uint8, win_begin int32, win_end int32, scores int32, sinks int32 [R, 2]); unaligned reads get the empty window"""
    torch = _torch()
    n, dev = best.shape[0], best.device
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    wb = torch.empty(n, dtype=torch.int32, device=dev); we = torch.empty(n, dtype=torch.int32, device=dev)
    scores = torch.empty(n, dtype=torch.int32, device=dev); sinks = torch.empty((n, 2), dtype=torch.int32, device=dev)
    if read_offsets is not None:                     # ragged reads (read_len / min_score are ignored)
        _check(lib().nvbio_traceback_best_batch_ragged(FMIndex._dev_index(dev), _ptr(best), _ptr(best_wb), n, _ptr(read_offsets), band, genome_len,
                                                       _ptr(min_scores), _ptr(flags), _ptr(wb), _ptr(we), _ptr(scores), _ptr(sinks),
                                                       _stream_ptr(dev)))
        return flags, wb, we, scores, sinks
    _check(lib().nvbio_traceback_best_batch(FMIndex._dev_index(dev), _ptr(best), _ptr(best_wb), n, read_len, band, genome_len, min_score, _ptr(flags),
                                            _ptr(wb), _ptr(we), _ptr(scores), _ptr(sinks), _stream_ptr(dev)))
    return flags, wb, we, scores, sinks


PE_POLICY_FF, PE_POLICY_FR, PE_POLICY_RF, PE_POLICY_RR = 0, 1, 2, 3


def max_text_gaps(scheme, min_score, pattern_len):
    """aln::max_text_gaps for a Gotoh aligner (nvbio/alignment/utils_inl.h:141-162): the largest number of reference
    gaps an alignment of pattern_len symbols can hold without dropping below min_score"""
    c = scheme.c
    score = pattern_len * c.match
    if score < min_score:
        return 0
    score += c.txt_gap_open
    n = 0
    while score >= min_score and n < pattern_len:
        score += c.txt_gap_ext
        n += 1
    return (n - 1) & 0xFFFFFFFF


class _MapqParams(ctypes.Structure):
    _fields_ = [("version", ctypes.c_int32), ("monotone", ctypes.c_int32), ("perfect_score", ctypes.c_int32),
                ("min_score", ctypes.c_int32)]


def second_candidate_reduce(keys, scores, sinks, wb, best, distinct_dist, worst_score, second, read_offsets=None, min_scores=None):
    """nvBowtie's second-best alignment per read (score_reduce, reduce_inl.h:65-140; see nvbio_second_candidate_reduce):
    best must already hold the final per-read maxima over ALL candidates; second is zero-initialised by the caller"""
    if read_offsets is not None:                     # ragged reads: distinct_dist = read_len / 2 and worst_score = min_score - 1 per read
        _check(lib().nvbio_second_candidate_reduce_ragged(FMIndex._dev_index(keys.device), _ptr(keys), _ptr(scores), _ptr(sinks), _ptr(wb),
                                                          keys.shape[0], _ptr(best), _ptr(read_offsets), _ptr(min_scores), _ptr(second),
                                                          _stream_ptr(keys.device)))
        return second
    _check(lib().nvbio_second_candidate_reduce(FMIndex._dev_index(keys.device), _ptr(keys), _ptr(scores), _ptr(sinks), _ptr(wb), keys.shape[0],
                                               _ptr(best), distinct_dist, worst_score, _ptr(second), _stream_ptr(keys.device)))
    return second


def mapq(best, second, perfect_score, min_score, monotone, version=2, read_offsets=None, min_scores=None, match=0):
    """Bowtie2's mapping quality per read from the best / second-best selection keys (BowtieMapq2 / BowtieMapq3,
    nvBowtie/bowtie2/cuda/mapq.h) -> (mapq uint8 [R], second_score int32 [R])"""
    torch = _torch()
    R = best.shape[0]
    q = torch.empty(R, dtype=torch.uint8, device=best.device)
    ss = torch.empty(R, dtype=torch.int32, device=best.device)
    if read_offsets is not None:                     # ragged reads: perfect score = match x length, min score per read
        _check(lib().nvbio_mapq_ragged(FMIndex._dev_index(best.device), _ptr(best), _ptr(second) if second is not None else None, R, int(version),
                                       int(match), _ptr(read_offsets), _ptr(min_scores), _ptr(ss), _ptr(q), _stream_ptr(best.device)))
        return q, ss
    prm = _MapqParams(int(version), 1 if monotone else 0, int(perfect_score), int(min_score))
    _check(lib().nvbio_mapq(FMIndex._dev_index(best.device), _ptr(best), _ptr(second) if second is not None else None, R, ctypes.byref(prm), _ptr(ss),
                            _ptr(q), _stream_ptr(best.device)))
    return q, ss


class FinishStatus:
    """the device status word of finish_reads calls on one device and its way to the host: the kernel ORs 1 into the word when the candidate
    list is not in tile order; every call copies the word to pinned memory behind its kernel.  check() raises if a call that has finished
    reported it (wait = True: after waiting for all of them) -- a pipelined caller looks where it synchronises anyway."""
    _per_device = {}

    @classmethod
    def of(cls, device):
        st = cls._per_device.get(str(device))
        if st is None:
            st = cls._per_device[str(device)] = cls(device)
        return st

    def __init__(self, device):
        torch = _torch()
        self.word = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(8, dtype=torch.int32, pin_memory=True)
        self.pending, self.slot = [], 0

    def record(self):
        torch = _torch()
        if len(self.pending) == self.host.numel():                   # every slot in flight: the oldest has to land first
            self.check(wait=True)
        i = self.slot
        self.slot = (i + 1) % self.host.numel()
        self.host[i:i + 1].copy_(self.word, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((ev, i))

    def check(self, wait=False):
        bad = False
        while self.pending and (wait or self.pending[0][0].query()):
            ev, i = self.pending.pop(0)
            ev.synchronize()
            bad = bad or int(self.host[i]) != 0
        if bad:
            self.pending = []
            _torch().cuda.synchronize(self.word.device)
            self.word.zero_()
            raise RuntimeError("finish_reads: the candidate list is not in tile order (a candidate outside its tile's span, or offsets that "
                               "do not cover the list): its outputs are invalid")


def finish_reads(keys, scores, sinks, wb, tile_offsets, reads_per_tile, n_reads, distinct_dist, worst_score, perfect_score, min_score, monotone,
                 version=2, read_offsets=None, min_scores=None, match=0, check=True):
    """nvbio_finish_reads: best_candidate_reduce + best_candidate_unpack + second_candidate_reduce + mapq of a candidate list in tile order (tile t
    = the reads [t * reads_per_tile, (t + 1) * reads_per_tile), its candidates = entries [tile_offsets[t], tile_offsets[t + 1]) of the list) in
    one launch -> dict(best, second, best_score, best_pos, best_rc, mapq, second_score).  A list that is not in tile order is reported by the
    device: check = True waits for the call and raises; check = False leaves that to FinishStatus.of( device ).check()."""
    torch = _torch()
    dev, R = tile_offsets.device, int(n_reads)
    n_tiles = int(tile_offsets.numel()) - 1
    out = dict(best=torch.empty(R, dtype=torch.int64, device=dev), second=torch.empty(R, dtype=torch.int64, device=dev),
               best_score=torch.empty(R, dtype=torch.int32, device=dev), best_pos=torch.empty(R, dtype=torch.int64, device=dev),
               best_rc=torch.empty(R, dtype=torch.uint8, device=dev), mapq=torch.empty(R, dtype=torch.uint8, device=dev),
               second_score=torch.empty(R, dtype=torch.int32, device=dev))
    if R == 0:
        return out
    st = FinishStatus.of(dev)
    prm = _MapqParams(int(version), 1 if monotone else 0, int(perfect_score), int(min_score))
    n = int(keys.numel())
    _check(lib().nvbio_finish_reads(
        FMIndex._dev_index(dev), _ptr(keys) if n else None, _ptr(scores) if n else None, _ptr(sinks) if n else None, _ptr(wb) if n else None, n,
        _ptr(tile_offsets), n_tiles, int(reads_per_tile), R, int(distinct_dist), int(worst_score), ctypes.byref(prm), int(match),
        _ptr(read_offsets) if read_offsets is not None else None, _ptr(min_scores) if min_scores is not None else None, _ptr(out["best"]),
        _ptr(out["second"]), _ptr(out["best_score"]), _ptr(out["best_pos"]), _ptr(out["best_rc"]), _ptr(out["mapq"]), _ptr(out["second_score"]),
        _ptr(st.word), _stream_ptr(dev)))
    st.record()
    if check:
        st.check(wait=True)
    return out


def opposite_mate_windows(g_pos, anchor_rc, anchor_len, opposite_gapped_len, anchor, genome_len, policy=PE_POLICY_FR,
                          min_frag_len=0, max_frag_len=500, overlap=True):
    """BestOppositeScoreStream::init_context's window (nvBowtie score_inl.h:389-425): (win_begin, win_end, flags, valid)"""
    torch = _torch()
    n, dev = g_pos.shape[0], g_pos.device
    wb = torch.empty(n, dtype=torch.int32, device=dev); we = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev); valid = torch.empty(n, dtype=torch.uint8, device=dev)
    _check(lib().nvbio_opposite_mate_windows(
        FMIndex._dev_index(dev), _ptr(g_pos), _ptr(anchor_rc), n, anchor_len, opposite_gapped_len, anchor, policy, min_frag_len, max_frag_len,
        1 if overlap else 0, genome_len, _ptr(wb), _ptr(we), _ptr(flags), _ptr(valid), _stream_ptr(dev)))
    return wb, we, flags, valid


def diagonals_to_windows(keys, band, read_len, genome_len, read_offsets=None):
    """genome_infixes + nvBowtie's window rule: (read_id, flags, win_begin, win_end) of every candidate key"""
    torch = _torch()
    n, dev = keys.numel(), keys.device
    rid = torch.empty(n, dtype=torch.int32, device=dev)
    fl = torch.empty(n, dtype=torch.uint8, device=dev)
    wb = torch.empty(n, dtype=torch.int32, device=dev)
    we = torch.empty(n, dtype=torch.int32, device=dev)
    if read_offsets is not None:                     # ragged reads: window end = begin + band + the read's own length
        _check(lib().nvbio_diagonals_to_windows_ragged(FMIndex._dev_index(dev), _ptr(keys), n, band, _ptr(read_offsets), genome_len, _ptr(rid),
                                                       _ptr(fl), _ptr(wb), _ptr(we), _stream_ptr(dev)))
        return rid, fl, wb, we
    _check(lib().nvbio_diagonals_to_windows(FMIndex._dev_index(dev), _ptr(keys), n, band, read_len, genome_len, _ptr(rid), _ptr(fl), _ptr(wb),
                                            _ptr(we), _stream_ptr(dev)))
    return rid, fl, wb, we


def text_2bit_le_to_be(words):
    """nvbio_text_2bit_le_to_be: 2-bit text words from sw-benchmark's little-endian packing to the library's big-endian one (int32 tensor)"""
    torch = _torch()
    out = torch.empty_like(words)
    _check(lib().nvbio_text_2bit_le_to_be(FMIndex._dev_index(words.device), _ptr(words), words.numel(), _ptr(out), _stream_ptr(words.device)))
    return out


def scores_to_int16(scores):
    """nvbio_scores_to_int16: int32 scores stored into int16, as sw-benchmark's output() stores them (the low 16 bits)"""
    torch = _torch()
    out = torch.empty(scores.numel(), dtype=torch.int16, device=scores.device)
    _check(lib().nvbio_scores_to_int16(FMIndex._dev_index(scores.device), _ptr(scores), scores.numel(), _ptr(out), _stream_ptr(scores.device)))
    return out


def u32(t):
    """int32 device/host tensor -> numpy uint32 (results are uint32 bit patterns)"""
    return t.detach().cpu().numpy().view(np.uint32)


# ---- nvBowtie's scoring stream as data (nvbio_hit_queues) ------------------------------------------------------------------------
class HitQueues:
    """the members of nvBowtie's scoring pipeline a BestScoreStream reads and writes (pipeline_states.h:49-115,
    scoring_queues.h:211-289), as int32 device tensors: idx_queue (or None), read_id, seed (packed_seed words), loc, score, sink"""

    def __init__(self, read_id, seed, loc, idx_queue=None, device="cuda:0"):
        torch = _torch()
        self.device = device
        self.read_id = _dev_tensor(read_id, torch.int32, device)
        self.seed = _dev_tensor(seed, torch.int32, device)
        self.loc = _dev_tensor(loc, torch.int32, device)
        self.idx_queue = _dev_tensor(idx_queue, torch.int32, device)
        self.n = int(self.idx_queue.numel() if self.idx_queue is not None else self.read_id.numel())     # may be lowered: the first n slots count
        self.score = torch.zeros(self.read_id.numel(), dtype=torch.int32, device=device)
        self.sink = torch.zeros(self.read_id.numel(), dtype=torch.int32, device=device)

    def c_struct(self):
        return _HitQueues(_ptr(self.idx_queue), _ptr(self.read_id), _ptr(self.seed), _ptr(self.loc), _ptr(self.score), _ptr(self.sink), self.n)


def score_stream_flatten(hits, read_index, band_len, genome_len, reads_reversed=True):
    """BestScoreStream::init_context + load_strings' orientation for the whole stream (nvbio_score_stream_flatten) ->
    (read_id, flags, win_begin, win_end): the per-job arrays of an AlignmentBatch"""
    torch = _torch()
    dev = hits.device
    ri = _dev_tensor(read_index, torch.int32, dev)
    rid = torch.empty(hits.n, dtype=torch.int32, device=dev)
    flags = torch.empty(hits.n, dtype=torch.uint8, device=dev)
    wb = torch.empty(hits.n, dtype=torch.int32, device=dev)
    we = torch.empty(hits.n, dtype=torch.int32, device=dev)
    hq = hits.c_struct()
    _check(lib().nvbio_score_stream_flatten(FMIndex._dev_index(dev), ctypes.byref(hq), _ptr(ri), band_len, genome_len, 1 if reads_reversed else 0,
                                            _ptr(rid), _ptr(flags), _ptr(wb), _ptr(we), _stream_ptr(dev)))
    return rid, flags, wb, we


def score_stream_output(hits, scores, sinks, win_begin, worst_score=-65536):
    """BestScoreStream::output for the whole stream (nvbio_score_stream_output): fills hits.score / hits.sink"""
    hq = hits.c_struct()
    _check(lib().nvbio_score_stream_output(FMIndex._dev_index(hits.device), ctypes.byref(hq), _ptr(scores), _ptr(sinks), _ptr(win_begin), worst_score,
                                           _stream_ptr(hits.device)))


# ---- nvBowtie's seed-hit deques, selection and effort-limited reduction (include/nvbio_amd.h: nvbio_seed_hits_*) -----------------
class SeedHitsParams:
    """nvbio_seed_hits_params with nvBowtie's defaults (bowtie2_cuda_driver.cu:86-141)"""

    def __init__(self, seeds_per_read, seed_interval, seed_len, read_len, first_offset=0, max_hits=100, rep_seeds=1000, max_effort=15,
                 min_ext=30, max_ext=400):
        self.c = _SeedHitsParams(seeds_per_read, first_offset, seed_interval, seed_len, read_len, max_hits, rep_seeds, max_effort, min_ext, max_ext)

    def capacity(self):
        cap = ctypes.c_uint32(0)
        _check(lib().nvbio_seed_hits_capacity(self.c.seeds_per_read, self.c.max_hits, ctypes.byref(cap)))
        return cap.value


def seed_hits_map(fw_ranges, rc_ranges, params, n_reads, deques, sizes, reseed=None, read_queue=None):
    """the exact seed mapper's deque bookkeeping (nvbio_seed_hits_map): fills deques [R, capacity, 2], sizes [R], reseed [R] for the
    n_reads reads of read_queue (None: reads 0..n_reads-1)"""
    dev = deques.device
    _check(lib().nvbio_seed_hits_map(FMIndex._dev_index(dev), _ptr(fw_ranges), _ptr(rc_ranges), _ptr(read_queue), n_reads, ctypes.byref(params.c),
                                     _ptr(deques), _ptr(sizes), _ptr(reseed), _stream_ptr(dev)))


def seed_hits_approx_capacity(params):
    cap = ctypes.c_uint32(0)
    _check(lib().nvbio_seed_hits_approx_capacity(params.c.seeds_per_read, params.c.seed_len, params.c.max_hits, ctypes.byref(cap)))
    return cap.value


def seed_hits_map_approx(fmi, rfmi, reads, read_bits, params, n_reads, deques, sizes, reseed=None, read_queue=None):
    """nvBowtie's approximate seed mapper (nvbio_seed_hits_map_approx): fmi = the forward index, rfmi = the index of the reversed text;
    reads = the stored (reversed) reads of params.read_len symbols back to back; deques [R, seed_hits_approx_capacity, 2]"""
    dev = deques.device
    _check(lib().nvbio_seed_hits_map_approx(fmi._h, rfmi._h, _ptr(reads), read_bits, _ptr(read_queue), n_reads, ctypes.byref(params.c), _ptr(deques),
                                            _ptr(sizes), _ptr(reseed), _stream_ptr(dev)))


def seed_hits_select(active, trys, params, deques, sizes, hits, active_out, count):
    """select_kernel (nvbio_seed_hits_select): active int32 [n] (read | top_flag << 31); fills hits.read_id / loc / seed and active_out;
    count int32 [1] on the device receives the number of slots written"""
    dev = deques.device
    hq = hits.c_struct()
    _check(lib().nvbio_seed_hits_select(FMIndex._dev_index(dev), _ptr(active), active.numel(), _ptr(trys), params.capacity(), _ptr(deques),
                                        _ptr(sizes), _ptr(active_out), ctypes.byref(hq), _ptr(count), _stream_ptr(dev)))


def seed_hits_loc(positions, hits):
    hq = hits.c_struct()
    _check(lib().nvbio_seed_hits_loc(FMIndex._dev_index(hits.device), _ptr(positions), ctypes.byref(hq), _stream_ptr(hits.device)))


def score_reduce_effort(active, hits, read_len, n_ext, params, best, best_rc, trys, sizes):
    """score_reduce_kernel with the best-approx effort rules (nvbio_score_reduce_effort): best int32 [R, 4] = (a1 score, a1 locus,
    a2 score, a2 locus), best_rc uint8 [R], trys int32 [R], sizes int32 [R] (erased deques get 0)"""
    hq = hits.c_struct()
    _check(lib().nvbio_score_reduce_effort(FMIndex._dev_index(hits.device), _ptr(active), ctypes.byref(hq), read_len, n_ext, ctypes.byref(params.c),
                                           _ptr(best), _ptr(best_rc), _ptr(trys), _ptr(sizes), _stream_ptr(hits.device)))


# ---- the same calls over reads of different lengths (include/nvbio_amd.h: nvbio_ragged_seed_layout and the *_ragged calls) -------------
class RaggedSeedLayout:
    """nvbio_ragged_seed_layout: the seeds of a seeding pass over a ragged batch -- read_offsets int32 [R + 1], seed_intervals int32 [R]
    (S_r = seed_freq( M_r )), seeds_per_read = the largest seed count of the pass (the stride of the per-seed arrays)"""

    def __init__(self, read_offsets, seed_intervals, seeds_per_read, seeding_pass, max_reseed, seed_len, min_read_len=12):
        self.read_offsets, self.seed_intervals = read_offsets, seed_intervals          # kept alive
        self.c = _RaggedSeedLayout(_ptr(read_offsets), _ptr(seed_intervals), seeds_per_read, seeding_pass, max_reseed, seed_len, min_read_len)


def read_queue_begin_ragged(queue, n, layout, n_symbols, top_seed, max_effort_init, seed_offsets=None, active=None, trys=None):
    """nvbio_read_queue_begin_ragged: seed_offsets int32 [n * seeds_per_read] (one explicit offset per seed slot), active int32 [n], trys int32 [R]"""
    dev = layout.read_offsets.device
    _check(lib().nvbio_read_queue_begin_ragged(FMIndex._dev_index(dev), _ptr(queue), n, ctypes.byref(layout.c), n_symbols, top_seed, max_effort_init,
                                               _ptr(seed_offsets), _ptr(active), _ptr(trys), _stream_ptr(dev)))


def seed_hits_map_ragged(fw_ranges, rc_ranges, layout, n_reads, max_hits, rep_seeds, deques, sizes, reseed=None, read_queue=None):
    """nvbio_seed_hits_map_ragged: the exact mapper's deques for the n_reads reads of read_queue (None: reads 0..n_reads-1) of a ragged batch"""
    dev = deques.device
    _check(lib().nvbio_seed_hits_map_ragged(FMIndex._dev_index(dev), _ptr(fw_ranges), _ptr(rc_ranges), _ptr(read_queue), n_reads,
                                            ctypes.byref(layout.c), max_hits, rep_seeds, _ptr(deques), _ptr(sizes), _ptr(reseed), _stream_ptr(dev)))


def best_approx_init_ragged(min_scores, best, best_rc):
    """nvbio_best_approx_init_ragged: best int32 [R, 4] = (min_scores[r], -1, min_scores[r], -1), best_rc uint8 [R] = 0"""
    dev = best.device
    _check(lib().nvbio_best_approx_init_ragged(FMIndex._dev_index(dev), best.shape[0], _ptr(min_scores), _ptr(best), _ptr(best_rc), _stream_ptr(dev)))


def score_reduce_effort_ragged(active, hits, read_offsets, n_ext, params, best, best_rc, trys, sizes):
    """nvbio_score_reduce_effort_ragged: score_reduce_effort with every read's own length (read_offsets int32 [R + 1]) in `distinct`"""
    hq = hits.c_struct()
    _check(lib().nvbio_score_reduce_effort_ragged(FMIndex._dev_index(hits.device), _ptr(active), ctypes.byref(hq), _ptr(read_offsets), n_ext,
                                                  ctypes.byref(params.c), _ptr(best), _ptr(best_rc), _ptr(trys), _ptr(sizes), _stream_ptr(hits.device)))


def score_reduce_effort_multi_ragged(active, n_active, hits_first, hits_count, hits, read_offsets, n_ext, params, best, best_rc, trys, sizes):
    """nvbio_score_reduce_effort_multi_ragged: the several-hits-per-read reduction over a ragged batch"""
    hq = hits.c_struct()
    _check(lib().nvbio_score_reduce_effort_multi_ragged(FMIndex._dev_index(hits.device), _ptr(active), n_active, _ptr(hits_first), _ptr(hits_count),
                                                        ctypes.byref(hq), _ptr(read_offsets), n_ext, ctypes.byref(params.c), _ptr(best),
                                                        _ptr(best_rc), _ptr(trys), _ptr(sizes), _stream_ptr(hits.device)))


# ---- the paired loop's steps over mates of different lengths (include/nvbio_amd.h: nvbio_pe_ragged and the nvbio_pe_*_ragged calls) ----
class _PeParams(ctypes.Structure):
    _fields_ = [("anchor", ctypes.c_uint32), ("anchor_len", ctypes.c_uint32), ("opposite_len", ctypes.c_uint32)] + \
               [(n, ctypes.c_int32) for n in ("anchor_perfect_score", "opposite_perfect_score", "anchor_min_score", "opposite_min_score", "score_limit",
                                              "worst_score", "match", "txt_gap_open", "txt_gap_ext")] + \
               [(n, ctypes.c_uint32) for n in ("band", "genome_len", "policy", "min_frag_len", "max_frag_len", "overlap", "unpaired", "max_effort", "min_ext",
                                               "max_ext")]


class _PeRagged(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("anchor_offsets_dev", "opposite_offsets_dev", "min_scores_mate1_dev", "min_scores_mate2_dev")]


class PeRaggedParams:
    """nvbio_pe_params as the ragged calls read it (the uniform lengths and scores stay 0: they are ignored) with nvBowtie's defaults"""

    def __init__(self, anchor, scheme, genome_len, band=31, policy=1, min_frag_len=0, max_frag_len=500, overlap=True, unpaired=True, max_effort=15,
                 min_ext=30, max_ext=400, score_limit=-(1 << 30)):
        self.c = _PeParams(anchor, 0, 0, 0, 0, 0, 0, score_limit, -65536, scheme.c.match, scheme.c.txt_gap_open, scheme.c.txt_gap_ext, band, genome_len, policy,
                           min_frag_len, max_frag_len, 1 if overlap else 0, 1 if unpaired else 0, max_effort, min_ext, max_ext)


class PeParams(PeRaggedParams):
    """nvbio_pe_params as the uniform calls read it: one length per mate, perfect_score( len ) = match * len and the two min scores"""

    def __init__(self, anchor, scheme, genome_len, anchor_len, opposite_len, anchor_min_score, opposite_min_score, **kw):
        super().__init__(anchor, scheme, genome_len, **kw)
        self.c.anchor_len, self.c.opposite_len = anchor_len, opposite_len
        self.c.anchor_perfect_score, self.c.opposite_perfect_score = scheme.c.match * anchor_len, scheme.c.match * opposite_len
        self.c.anchor_min_score, self.c.opposite_min_score = anchor_min_score, opposite_min_score


class PeRagged:
    """nvbio_pe_ragged: the anchor / opposite mate's offsets int32 [R + 1] (by ROLE) and min_score( len ) of every mate 1 / mate 2 int32 [R] (by MATE)"""

    def __init__(self, anchor_offsets, opposite_offsets, min_scores_mate1, min_scores_mate2):
        self.tensors = (anchor_offsets, opposite_offsets, min_scores_mate1, min_scores_mate2)          # kept alive
        self.c = _PeRagged(*[_ptr(t) for t in self.tensors])


def pe_init_ragged(ragged, best_a, best_o):
    """nvbio_pe_init_ragged: best_a / best_o int32 [R, 2, 4] = unaligned at min_scores_mate1[r] / min_scores_mate2[r]"""
    dev = best_a.device
    _check(lib().nvbio_pe_init_ragged(FMIndex._dev_index(dev), best_a.shape[0], ctypes.byref(ragged.c), _ptr(best_a), _ptr(best_o), _stream_ptr(dev)))


def pe_anchor_flatten_ragged(params, ragged, hits, best_a, best_o, read_id, flags, win_begin, win_end, min_scores):
    """nvbio_pe_anchor_flatten_ragged: the per-job arrays of the anchor's banded DP (int32 [hits.n], flags uint8) and the hits' min scores"""
    hq = hits.c_struct()
    _check(lib().nvbio_pe_anchor_flatten_ragged(FMIndex._dev_index(hits.device), ctypes.byref(params.c), ctypes.byref(ragged.c), ctypes.byref(hq), _ptr(best_a),
                                                _ptr(best_o), _ptr(read_id), _ptr(flags), _ptr(win_begin), _ptr(win_end), _ptr(min_scores),
                                                _stream_ptr(hits.device)))


def pe_opposite_flatten_ragged(params, ragged, queue, n, hits, best_a, best_o, read_id, flags, win_begin, win_end, min_scores):
    """nvbio_pe_opposite_flatten_ragged: the same for the opposite mate of the n hits of queue (those whose anchor passed)"""
    hq = hits.c_struct()
    _check(lib().nvbio_pe_opposite_flatten_ragged(FMIndex._dev_index(hits.device), ctypes.byref(params.c), ctypes.byref(ragged.c), _ptr(queue), n,
                                                  ctypes.byref(hq), _ptr(best_a), _ptr(best_o), _ptr(read_id), _ptr(flags), _ptr(win_begin), _ptr(win_end),
                                                  _ptr(min_scores), _stream_ptr(hits.device)))


def pe_score_reduce_ragged(params, ragged, active, n_active, hits_first, hits_count, hits, hit_oscore, hit_oloc, hit_osink, n_ext, best_a, best_o, trys, sizes):
    """nvbio_pe_score_reduce_ragged: score_reduce_paired with the anchor read's own length in `distinct`"""
    hq = hits.c_struct()
    _check(lib().nvbio_pe_score_reduce_ragged(FMIndex._dev_index(hits.device), ctypes.byref(params.c), ctypes.byref(ragged.c), _ptr(active), n_active,
                                              _ptr(hits_first), _ptr(hits_count), ctypes.byref(hq), _ptr(hit_oscore), _ptr(hit_oloc), _ptr(hit_osink),
                                              n_ext, _ptr(best_a), _ptr(best_o), _ptr(trys), _ptr(sizes), _stream_ptr(hits.device)))


def pe_init(worst_score_mate1, worst_score_mate2, best_a, best_o):
    """nvbio_pe_init: best_a / best_o int32 [R, 2, 4] = unaligned at the two mates' min scores"""
    dev = best_a.device
    _check(lib().nvbio_pe_init(FMIndex._dev_index(dev), best_a.shape[0], worst_score_mate1, worst_score_mate2, _ptr(best_a), _ptr(best_o), _stream_ptr(dev)))


def pe_anchor_flatten(params, hits, best_a, best_o, read_id, flags, win_begin, win_end, min_scores):
    """nvbio_pe_anchor_flatten: the per-job arrays of the anchor's banded DP (int32 [hits.n], flags uint8) and the hits' min scores"""
    hq = hits.c_struct()
    _check(lib().nvbio_pe_anchor_flatten(FMIndex._dev_index(hits.device), ctypes.byref(params.c), ctypes.byref(hq), _ptr(best_a), _ptr(best_o), _ptr(read_id),
                                         _ptr(flags), _ptr(win_begin), _ptr(win_end), _ptr(min_scores), _stream_ptr(hits.device)))


def pe_anchor_output(params, hits, scores, sinks, win_begin, min_scores, hit_oscore, valid):
    """nvbio_pe_anchor_output (serves both forms): fills hits.score / hits.sink, hit_oscore int32 [hits.n] = worst_score, valid uint8 [hits.n]"""
    hq = hits.c_struct()
    _check(lib().nvbio_pe_anchor_output(FMIndex._dev_index(hits.device), ctypes.byref(params.c), ctypes.byref(hq), _ptr(scores), _ptr(sinks), _ptr(win_begin),
                                        _ptr(min_scores), _ptr(hit_oscore), _ptr(valid), _stream_ptr(hits.device)))


def pe_opposite_flatten(params, queue, n, hits, best_a, best_o, read_id, flags, win_begin, win_end, min_scores):
    """nvbio_pe_opposite_flatten: the same for the opposite mate of the n hits of queue (those whose anchor passed)"""
    hq = hits.c_struct()
    _check(lib().nvbio_pe_opposite_flatten(FMIndex._dev_index(hits.device), ctypes.byref(params.c), _ptr(queue), n, ctypes.byref(hq), _ptr(best_a), _ptr(best_o),
                                           _ptr(read_id), _ptr(flags), _ptr(win_begin), _ptr(win_end), _ptr(min_scores), _stream_ptr(hits.device)))


def pe_opposite_output(params, queue, n, scores, sinks, win_begin, win_end, min_scores, hit_oscore, hit_oloc, hit_osink):
    """nvbio_pe_opposite_output (serves both forms): the opposite score, window begin and sink of the hits queue names"""
    dev = scores.device
    _check(lib().nvbio_pe_opposite_output(FMIndex._dev_index(dev), ctypes.byref(params.c), _ptr(queue), n, _ptr(scores), _ptr(sinks), _ptr(win_begin),
                                          _ptr(win_end), _ptr(min_scores), _ptr(hit_oscore), _ptr(hit_oloc), _ptr(hit_osink), _stream_ptr(dev)))


def pe_score_reduce(params, active, n_active, hits_first, hits_count, hits, hit_oscore, hit_oloc, hit_osink, n_ext, best_a, best_o, trys, sizes):
    """nvbio_pe_score_reduce: score_reduce_paired over every active read's hits"""
    hq = hits.c_struct()
    _check(lib().nvbio_pe_score_reduce(FMIndex._dev_index(hits.device), ctypes.byref(params.c), _ptr(active), n_active, _ptr(hits_first), _ptr(hits_count),
                                       ctypes.byref(hq), _ptr(hit_oscore), _ptr(hit_oloc), _ptr(hit_osink), n_ext, _ptr(best_a), _ptr(best_o), _ptr(trys),
                                       _ptr(sizes), _stream_ptr(hits.device)))


# ---- nvBowtie's all-mapping mode (include/nvbio_amd.h: nvbio_all_*; host/nvbio_amd/all_mapping.hpp) ---------------------------------
class _AllHitsParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("seeds_per_read", "first_offset", "seed_interval", "seed_len", "read_len")]


class AllHitsParams:
    """nvbio_all_hits_params: the seed layout of the all-mapping mode (seed j of a read at stored offset first_offset + j * seed_interval)"""

    def __init__(self, seeds_per_read, first_offset, seed_interval, seed_len, read_len):
        self.c = _AllHitsParams(seeds_per_read, first_offset, seed_interval, seed_len, read_len)


def band_length(max_dist):
    """Aligner::band_length (nvBowtie/bowtie2/cuda/aligner.h:149-158)"""
    band_len = 4
    while band_len - 1 < max_dist * 2 + 1:
        band_len *= 2
    return band_len - 1


def _temp_for(query, *args, device="cuda:0"):
    b = ctypes.c_uint64(0)
    _check(query(*args, ctypes.byref(b)))
    return _torch().empty(max(int(b.value), 256), dtype=_torch().uint8, device=device), b.value


def all_hits_scan(fw_ranges, rc_ranges, n_reads, params):
    """gather_ranges + the scans of score_all (nvbio_all_hits_scan) -> (slots int64 [2 * n_reads * seeds_per_read], n_hits int64 [1]),
    both on the device: the inclusive scan of the range sizes in hit order and its total"""
    torch = _torch()
    dev = fw_ranges.device
    slots = torch.zeros(2 * n_reads * params.c.seeds_per_read, dtype=torch.int64, device=dev)
    n_hits = torch.zeros(1, dtype=torch.int64, device=dev)
    tmp, nb = _temp_for(lib().nvbio_all_hits_scan_temp_bytes, n_reads, params.c.seeds_per_read, device=dev)
    _check(lib().nvbio_all_hits_scan(FMIndex._dev_index(dev), _ptr(fw_ranges), _ptr(rc_ranges), n_reads, ctypes.byref(params.c), _ptr(slots),
                                     _ptr(n_hits), _ptr(tmp), nb, _stream_ptr(dev)))
    return slots, n_hits


def all_hits_select(fw_ranges, rc_ranges, n_reads, params, slots, begin, end, hits):
    """select_all_kernel (nvbio_all_hits_select): fills hits.read_id / loc (the SA row) / seed for the hits [begin, end) of the scan"""
    dev = hits.device
    hq = hits.c_struct()
    _check(lib().nvbio_all_hits_select(FMIndex._dev_index(dev), _ptr(fw_ranges), _ptr(rc_ranges), n_reads, ctypes.byref(params.c), _ptr(slots), begin,
                                       end, ctypes.byref(hq), _stream_ptr(dev)))


def all_hits_unique(hits):
    """nvbio_all_hits_unique, in place: one located hit per distinct (read_id, rc, loc) at the front of the queues, in ascending order
    -> their number (hits.n is lowered to it)"""
    torch = _torch()
    dev = hits.device
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    tmp, nb = _temp_for(lib().nvbio_all_hits_unique_temp_bytes, hits.n, device=dev)
    hq = hits.c_struct()
    _check(lib().nvbio_all_hits_unique(FMIndex._dev_index(dev), ctypes.byref(hq), ctypes.byref(hq), _ptr(n_out), _ptr(tmp), nb, _stream_ptr(dev)))
    hits.n = int(n_out.item())
    return hits.n


def all_score_output(hits, scores, min_score, out, out_offset, count):
    """AllScoreStream::output (nvbio_all_score_output): appends (read_id, rc, loc, score) of the hits with score >= min_score to
    out = (read_id int32, rc uint8, loc int32, score int32) from slot out_offset on, in hit order; count int64 [1] += the number accepted"""
    dev = hits.device
    tmp, nb = _temp_for(lib().nvbio_all_score_output_temp_bytes, hits.n, device=dev)
    hq = hits.c_struct()
    _check(lib().nvbio_all_score_output(FMIndex._dev_index(dev), ctypes.byref(hq), _ptr(scores), min_score, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                        _ptr(out[3]), out_offset, out[0].numel(), _ptr(count), _ptr(tmp), nb, _stream_ptr(dev)))


def all_traceback_flatten(rec_read_id, rec_rc, rec_loc, read_index, band_len, genome_len, reads_reversed=True):
    """AllTracebackStream::init_context (nvbio_all_traceback_flatten) -> (read_id, flags, win_begin, win_end) of the accepted records"""
    torch = _torch()
    dev = rec_read_id.device
    n = rec_read_id.numel()
    ri = _dev_tensor(read_index, torch.int32, dev)
    rid = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    wb = torch.empty(n, dtype=torch.int32, device=dev)
    we = torch.empty(n, dtype=torch.int32, device=dev)
    _check(lib().nvbio_all_traceback_flatten(FMIndex._dev_index(dev), _ptr(rec_read_id), _ptr(rec_rc), _ptr(rec_loc), n, _ptr(ri), band_len,
                                             genome_len, 1 if reads_reversed else 0, _ptr(rid), _ptr(flags), _ptr(wb), _ptr(we), _stream_ptr(dev)))
    return rid, flags, wb, we


class _AllMappingParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("seed_len", "seed_freq", "max_reseed", "max_dist", "band", "aln_type", "hits_per_batch", "unique",
                                                "per_seed_passes", "want_cigars")]


class _AllMappingOutput(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_uint64)] + [(n, ctypes.c_void_p) for n in ("read_id", "rc", "loc", "score", "win_begin", "source", "sink", "ed",
                                                                                  "cigars", "cigar_lens", "mds", "mds_lens")] + \
               [("cigar_stride", ctypes.c_uint32), ("mds_stride", ctypes.c_uint32)]


class _AllMappingStats(ctypes.Structure):
    _fields_ = [("n_hits", ctypes.c_uint64), ("n_scored", ctypes.c_uint64), ("n_alignments", ctypes.c_uint64), ("chunks", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


class AllMappingParams:
    """AllMappingParams of host/nvbio_amd/all_mapping.hpp with nvBowtie's defaults; min_score defaults to -max_dist and the scheme to the
    edit-distance one (0, -1, -1, -1): the mode as the reference ships it"""

    def __init__(self, seed_len=22, seed_freq=0, max_reseed=2, max_dist=15, band=0, aln_type=SEMI_GLOBAL, hits_per_batch=0, unique=False,
                 per_seed_passes=False, scheme=(0, -1, -1, -1), min_score=None):
        self.seed_len, self.seed_freq, self.max_reseed, self.max_dist, self.band = seed_len, seed_freq, max_reseed, max_dist, band
        self.aln_type, self.hits_per_batch, self.unique, self.per_seed_passes = aln_type, hits_per_batch, unique, per_seed_passes
        self.scheme, self.min_score = tuple(scheme), (-max_dist if min_score is None else min_score)


def all_mapping(fmi, genome2, genome_len, stored_reads4, n_reads, read_len, params, capacity, want_cigars=False, cigar_stride=64, mds_stride=0):
    """nvBowtie's all-mapping mode (Aligner::all, aligner_all.h:29-485) through the C++ host loop nvbio_host_all_mapping: every alignment of
    every read that reaches params.min_score.  stored_reads4: the reads as nvBowtie stores them (reversed), 4-bit packed, back to back.
    -> dict(read_id, rc, loc, score [+ win_begin, source, sink, ed, cigars, cigar_lens (, mds, mds_lens)]: device tensors cut to
    min(n_alignments, capacity) records; n_hits, n_scored, n_alignments, chunks)"""
    torch = _torch()
    from .pipeline import _host_lib
    dev = fmi.device
    cap = int(capacity)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    out = dict(read_id=i32(cap), rc=torch.zeros(cap, dtype=torch.uint8, device=dev), loc=i32(cap), score=i32(cap))
    if want_cigars:
        out.update(win_begin=i32(cap), source=i32(cap, 2), sink=i32(cap, 2), ed=i32(cap), cigars=torch.zeros((cap, cigar_stride), dtype=torch.int16, device=dev),
                   cigar_lens=i32(cap))
        if mds_stride:
            out.update(mds=torch.zeros((cap, mds_stride), dtype=torch.uint8, device=dev), mds_lens=i32(cap))
    o = _AllMappingOutput(cap, *[_ptr(out.get(k)) for k in ("read_id", "rc", "loc", "score", "win_begin", "source", "sink", "ed", "cigars", "cigar_lens",
                                                            "mds", "mds_lens")], cigar_stride if want_cigars else 0, mds_stride if want_cigars else 0)
    p = _AllMappingParams(params.seed_len, params.seed_freq, params.max_reseed, params.max_dist, params.band, int(params.aln_type), params.hits_per_batch,
                          1 if params.unique else 0, 1 if params.per_seed_passes else 0, 1 if want_cigars else 0)
    sw = _SWScheme(*params.scheme)
    st = _AllMappingStats()
    reads = _dev_tensor(stored_reads4, torch.int32, dev)
    rc = _host_lib().nvbio_host_all_mapping(FMIndex._dev_index(dev), fmi._h, _ptr(genome2), genome_len, _ptr(reads), n_reads, read_len,
                                            ctypes.byref(sw), params.min_score, ctypes.byref(p), ctypes.byref(o), _stream_ptr(dev), ctypes.byref(st))
    if rc != 0:
        raise RuntimeError(_host_lib().nvbio_host_last_error().decode())
    k = min(int(st.n_alignments), cap)
    res = {name: t[:k] for name, t in out.items()}
    res.update(n_hits=int(st.n_hits), n_scored=int(st.n_scored), n_alignments=int(st.n_alignments), chunks=int(st.chunks))
    return res


# ---- the generic rank dictionary (nvbio_rank_dictionary_*) -------------------------------------------------------------------------
class RankDictionary:
    """nvbio::rank_dictionary<2, K, PackedStream<const uint32*|const uint64*, uint8, 2, true>, occ, count_table> over plain word storage
    with a separate occurrence table and 32- or 64-bit indices (nvbio/fmindex/rank_dictionary_inl.h:206-336).  text: int32 tensor of
    32-bit words or int64 tensor of 64-bit words (bit patterns), on the device."""

    def __init__(self, text, length, K, index_bits):
        torch = _torch()
        self.text, self.length, self.K, self.index_bits = text, int(length), int(K), int(index_bits)
        self.word_bits = 32 if text.dtype == torch.int32 else 64
        self.device = text.device
        d = self._c(None)
        n = ctypes.c_uint64(0)
        _check(lib().nvbio_rank_dictionary_occ_entries(ctypes.byref(d), ctypes.byref(n)))
        self.occ = torch.zeros(max(n.value, 4), dtype=torch.int32 if index_bits == 32 else torch.int64, device=self.device)
        counts = (ctypes.c_uint64 * 4)()
        _check(lib().nvbio_rank_dictionary_build(FMIndex._dev_index(self.device), ctypes.byref(d), _ptr(self.occ), counts, _stream_ptr(self.device)))
        self.counts = [int(c) for c in counts]

    def _c(self, occ):
        return _RankDict(_ptr(self.text), self.word_bits, _ptr(occ), self.index_bits, self.K, self.length)

    def rank(self, idx, syms):
        """idx: tensor of index_bits-wide indices; syms uint8 -> ranks (same dtype as idx)"""
        torch = _torch()
        out = torch.empty_like(idx)
        d = self._c(self.occ)
        _check(lib().nvbio_rank_dictionary_rank(FMIndex._dev_index(self.device), ctypes.byref(d), _ptr(idx), _ptr(syms), idx.numel(), _ptr(out),
                                                _stream_ptr(self.device)))
        return out

    def rank4(self, idx):
        torch = _torch()
        out = torch.empty((idx.numel(), 4), dtype=idx.dtype, device=idx.device)
        d = self._c(self.occ)
        _check(lib().nvbio_rank_dictionary_rank4(FMIndex._dev_index(self.device), ctypes.byref(d), _ptr(idx), idx.numel(), _ptr(out),
                                                 _stream_ptr(self.device)))
        return out


def batch_banded_myers_score(band, aln_type, batch, min_score=SCORE_MIN):
    """aln::batch_banded_alignment_score<BAND>( make_edit_distance_aligner<TYPE, MyersTag<5>>(), ... ) (nvbio_banded_myers_score): the aligner of
    examples/fmmap -> (scores = -(edit distance), sinks)"""
    torch = _torch()
    scores = torch.empty(batch.n, dtype=torch.int32, device=batch.device)
    sinks = torch.empty((batch.n, 2), dtype=torch.int32, device=batch.device)
    bs = batch.c_struct()
    _check(lib().nvbio_banded_myers_score(FMIndex._dev_index(batch.device), band, aln_type, ctypes.byref(bs), min_score, _ptr(scores), _ptr(sinks),
                                          _stream_ptr(batch.device)))
    return scores, sinks


# ---- SAM output ------------------------------------------------------------------------------------------------------------------
SAM_STATUS_CAPACITY, SAM_STATUS_OFFSETS, SAM_STATUS_TOO_LONG = 1, 2, 4
SAM_LENGTHS_ONLY = 1                                                     # sam_record_offsets: the lengths, not scanned
SAM_ALIGNED, SAM_RC, SAM_READ_2, SAM_PAIRED = 1, 2, 4, 8                # the bits of SamRecords.state


class _SamRefs(ctypes.Structure):
    _fields_ = [("n_seqs", ctypes.c_uint32), ("max_name_len", ctypes.c_uint32), ("sequence_index_dev", ctypes.c_void_p), ("names_dev", ctypes.c_void_p),
                ("names_index_dev", ctypes.c_void_p)]


class _SamRecords(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("n", "max_name_len", "max_read_len", "reads_reversed")] + \
               [(n, ctypes.c_void_p) for n in ("names_dev", "name_index_dev", "reads4_dev", "read_index_dev", "quals_dev", "state_dev", "pos_dev",
                                               "score_dev", "second_score_dev", "ed_dev", "mapq_dev", "cigars_dev", "cigar_lens_dev", "mds_dev",
                                               "mds_lens_dev", "mate_of_dev")] + \
               [("cigar_stride", ctypes.c_uint32), ("mds_stride", ctypes.c_uint32)]


def _name_table(names, device):
    """[bytes or str] -> (uint8 tensor of the names' bytes, int32 tensor of n + 1 offsets, the longest name's length)"""
    torch = _torch()
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    index = np.zeros(len(names) + 1, dtype=np.int64)
    index[1:] = np.cumsum([len(n) for n in names]) if names else 0
    data = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(data).to(device), torch.from_numpy(index.astype(np.int32)).to(device), max([len(n) for n in names] or [0])


class SamRefs:
    """nvbio_sam_refs: the reference sequences of the genome (io::ConstSequenceDataView / bnt): names ([bytes or str]) and sequence_index
    (n_seqs + 1 starts in the concatenated genome, [0] = 0)"""

    def __init__(self, names, sequence_index, device="cuda:0"):
        self.device = device
        self.names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        self.sequence_index_host = np.asarray(sequence_index, dtype=np.int64)
        assert len(self.sequence_index_host) == len(self.names) + 1
        self.sequence_index = _dev_tensor(self.sequence_index_host.astype(np.uint32), _torch().int32, device)
        self.names_data, self.names_index, self.max_name_len = _name_table(self.names, device)

    def c_struct(self):
        return _SamRefs(len(self.names), self.max_name_len, self.sequence_index.data_ptr(), self.names_data.data_ptr(), self.names_index.data_ptr())


class SamRecords:
    """nvbio_sam_records over device tensors (numpy arrays are uploaded): what a SAM record is printed from.
    names: [bytes or str] * n, or a (bytes tensor, offsets tensor, longest) triple already on the device; reads4 / read_index / quals: the STORED
    reads; state: uint8 (SAM_ALIGNED | SAM_RC | SAM_READ_2 | SAM_PAIRED); pos: where the alignment starts in the concatenated genome;
    cigars [n, cigar_stride] / cigar_lens as a traceback writes them; mds [n, mds_stride] / mds_lens as finish_alignment writes them;
    mate_of: the record index of each record's mate, or None (single-end)."""

    def __init__(self, names, reads4, read_index, max_read_len, state, pos, score, ed, mapq, cigars, cigar_lens, quals=None, second_score=None,
                 mds=None, mds_lens=None, mate_of=None, reads_reversed=True, device="cuda:0"):
        torch = _torch()
        self.device = device
        self.names_data, self.name_index, self.max_name_len = names if isinstance(names, tuple) else _name_table(names, device)
        self.n = int(self.name_index.numel()) - 1
        self.max_read_len, self.reads_reversed = int(max_read_len), bool(reads_reversed)
        t = lambda a, dtype: _dev_tensor(a, dtype, device)
        self.reads4, self.read_index, self.quals = t(reads4, torch.int32), t(read_index, torch.int32), t(quals, torch.uint8)
        self.state, self.pos, self.score, self.second_score = t(state, torch.uint8), t(pos, torch.int32), t(score, torch.int32), t(second_score, torch.int32)
        self.ed, self.mapq = t(ed, torch.int32), t(mapq, torch.uint8)
        self.cigars, self.cigar_lens = cigars.to(device).contiguous() if isinstance(cigars, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(cigars).view(np.int16)).to(device), t(cigar_lens, torch.int32)
        assert self.cigars.dim() == 2 and self.cigars.element_size() == 2 and self.cigars.shape[0] == self.n
        self.mds, self.mds_lens = t(mds, torch.uint8), t(mds_lens, torch.int32)
        assert self.mds is None or (self.mds.dim() == 2 and self.mds.shape[0] == self.n and self.mds_lens is not None)
        self.mate_of = t(mate_of, torch.int32)

    def c_struct(self):
        p = lambda x: None if x is None else x.data_ptr()
        return _SamRecords(self.n, self.max_name_len, self.max_read_len, 1 if self.reads_reversed else 0, p(self.names_data), p(self.name_index),
                           p(self.reads4), p(self.read_index), p(self.quals), p(self.state), p(self.pos), p(self.score), p(self.second_score), p(self.ed),
                           p(self.mapq), p(self.cigars), p(self.cigar_lens), p(self.mds), p(self.mds_lens), p(self.mate_of), self.cigars.shape[1],
                           0 if self.mds is None else self.mds.shape[1])


def sam_record_offsets(refs, records, flags=0):
    """nvbio_sam_record_offsets -> offsets int64 [n + 1] on the device: the exclusive scan of the records' bytes, [n] the total"""
    torch = _torch()
    dev = records.device
    offsets = torch.empty(records.n + 1, dtype=torch.int64, device=dev)
    tmp, nb = _temp_for(lib().nvbio_sam_format_temp_bytes, records.n, device=dev)
    rs, cs = refs.c_struct(), records.c_struct()
    _check(lib().nvbio_sam_record_offsets(FMIndex._dev_index(dev), ctypes.byref(rs), ctypes.byref(cs), flags, _ptr(offsets), _ptr(tmp), nb, _stream_ptr(dev)))
    return offsets


def sam_format(refs, records, offsets, text, flags=0):
    """nvbio_sam_format into `text` (a uint8 device tensor) -> (n_skipped, status): one host synchronisation"""
    torch = _torch()
    dev = records.device
    words = torch.zeros(2, dtype=torch.int32, device=dev)                  # n_skipped | status
    rs, cs = refs.c_struct(), records.c_struct()
    _check(lib().nvbio_sam_format(FMIndex._dev_index(dev), ctypes.byref(rs), ctypes.byref(cs), flags, _ptr(offsets), _ptr(text), text.numel(),
                                  ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(words.data_ptr() + 4), _stream_ptr(dev)))
    n_skipped, status = (int(v) for v in words.cpu().numpy())
    return n_skipped, status


def sam_records(refs, records, flags=0):
    """The SAM text of a batch of records (io::SamOutput, output_sam.cpp:182-544), formatted on the device: offsets, one read of the
    total, the text -> (text uint8 tensor [offsets[n]], offsets int64 tensor [n + 1], n_skipped); record i is text[offsets[i] :
    offsets[i + 1]], empty for a record that is skipped (a truncated or inconsistent CIGAR)"""
    torch = _torch()
    offsets = sam_record_offsets(refs, records, flags)
    total = int(offsets[-1].item())
    text = torch.empty(total, dtype=torch.uint8, device=records.device)
    n_skipped, status = sam_format(refs, records, offsets, text, flags)
    if status:
        raise NvbioError(1, "nvbio_sam_format: status %d (NVBIO_SAM_STATUS_*)" % status)
    return text, offsets, n_skipped


# ---- BAM output ------------------------------------------------------------------------------------------------------------------
BAM_STATUS_CAPACITY, BAM_STATUS_OFFSETS, BAM_STATUS_TOO_LONG = 1, 2, 4
BAM_LENGTHS_ONLY = 1                                                     # bam_record_offsets: the lengths, not scanned
BAM_REG2BIN = 2                                                          # bin = reg2bin(pos, pos + reference span) instead of the reference's 0
BGZF_BLOCK_BYTES, BGZF_OVERHEAD = 65280, 31
BGZF_EOF = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])   # output_bam.cpp:657-659


def bam_record_offsets(refs, records, flags=0):
    """nvbio_bam_record_offsets -> offsets int64 [n + 1] on the device: the exclusive scan of the records' bytes, [n] the total"""
    torch = _torch()
    dev = records.device
    offsets = torch.empty(records.n + 1, dtype=torch.int64, device=dev)
    tmp, nb = _temp_for(lib().nvbio_bam_format_temp_bytes, records.n, device=dev)
    rs, cs = refs.c_struct(), records.c_struct()
    _check(lib().nvbio_bam_record_offsets(FMIndex._dev_index(dev), ctypes.byref(rs), ctypes.byref(cs), flags, _ptr(offsets), _ptr(tmp), nb, _stream_ptr(dev)))
    return offsets


def bam_format(refs, records, offsets, data, flags=0):
    """nvbio_bam_format into `data` (a uint8 device tensor) -> (n_skipped, status): one host synchronisation"""
    torch = _torch()
    dev = records.device
    words = torch.zeros(2, dtype=torch.int32, device=dev)                  # n_skipped | status
    rs, cs = refs.c_struct(), records.c_struct()
    _check(lib().nvbio_bam_format(FMIndex._dev_index(dev), ctypes.byref(rs), ctypes.byref(cs), flags, _ptr(offsets), _ptr(data), data.numel(),
                                  ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(words.data_ptr() + 4), _stream_ptr(dev)))
    n_skipped, status = (int(v) for v in words.cpu().numpy())
    return n_skipped, status


def bam_records(refs, records, flags=0):
    """The BAM records of a batch (io::BamOutput, output_bam.cpp:227-544), made on the device: offsets, one read of the total, the bytes
    -> (data uint8 tensor [offsets[n]], offsets int64 tensor [n + 1], n_skipped); record i is data[offsets[i] : offsets[i + 1]], its
    block_size word first, empty for a record that is skipped (a truncated or inconsistent CIGAR).  flags: 0 or BAM_REG2BIN."""
    torch = _torch()
    offsets = bam_record_offsets(refs, records, flags)
    total = int(offsets[-1].item())
    data = torch.empty(total, dtype=torch.uint8, device=records.device)
    n_skipped, status = bam_format(refs, records, offsets, data, flags)
    if status:
        raise NvbioError(1, "nvbio_bam_format: status %d (NVBIO_BAM_STATUS_*)" % status)
    return data, offsets, n_skipped


def bgzf_framed_bytes(n):
    """nvbio_bgzf_framed_bytes: n + 31 for every block of at most 65280 bytes"""
    b = ctypes.c_uint64(0)
    _check(lib().nvbio_bgzf_framed_bytes(int(n), ctypes.byref(b)))
    return int(b.value)


def bgzf_frame(data):
    """nvbio_bgzf_frame: a uint8 device tensor (16-byte aligned; numpy arrays and bytes are uploaded to cuda:0) as BGZF blocks of stored
    DEFLATE blocks, each with its CRC-32 -> uint8 tensor [bgzf_framed_bytes(n)] on the same device; the EOF block (BGZF_EOF) is the caller's"""
    torch = _torch()
    if not isinstance(data, torch.Tensor):
        data = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to("cuda:0")
    data = data.contiguous()
    if data.data_ptr() & 15:
        data = data.clone()
    out = torch.empty(bgzf_framed_bytes(data.numel()), dtype=torch.uint8, device=data.device)
    _check(lib().nvbio_bgzf_frame(FMIndex._dev_index(data.device), _ptr(data), data.numel(), _ptr(out), out.numel(), _stream_ptr(data.device)))
    return out


# ---- FASTQ input -----------------------------------------------------------------------------------------------------------------
FASTQ_PHRED, FASTQ_PHRED33, FASTQ_PHRED64, FASTQ_SOLEXA = 0, 1, 2, 3
FASTQ_NO_OP, FASTQ_REVERSE_OP, FASTQ_COMPLEMENT_OP, FASTQ_REVERSE_COMPLEMENT_OP = 0, 1, 2, 3
FASTQ_STATUS_MARKER, FASTQ_STATUS_INCOMPLETE, FASTQ_STATUS_LENGTH, FASTQ_STATUS_EMPTY, FASTQ_STATUS_CAPACITY = 1, 2, 4, 8, 16
FASTQ_UNLIMITED = 0xFFFFFFFF
FASTQ_SUMMARY_FIELDS = ("n_records", "consumed_bytes", "n_symbols", "n_name_bytes", "max_read_len", "max_name_len", "status", "error_offset",
                        "error_char", "first_bad_record")


class _FastqParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("quality_encoding", "strand_op", "truncate_len", "max_records")]


class _FastqSummary(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in FASTQ_SUMMARY_FIELDS]


def _fastq_text(text, device):
    """bytes, numpy array or uint8 tensor -> a uint8 device tensor whose first byte is 16-byte aligned"""
    torch = _torch()
    if isinstance(text, torch.Tensor):
        t = text.to(device).contiguous().view(torch.uint8).reshape(-1)
        return t.clone() if t.numel() and t.data_ptr() & 15 else t
    a = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to(device)


def fastq_scan(text, params, temp=None, text_bytes=None):
    """nvbio_fastq_scan over a uint8 device tensor -> (summary: int32 tensor [10] on the device, FASTQ_SUMMARY_FIELDS; temp: what
    fastq_encode reads).  params: a _FastqParams.  text_bytes: the length to declare, when it is not the tensor's.  No synchronisation."""
    torch = _torch()
    dev = text.device
    nb = text.numel() if text_bytes is None else int(text_bytes)
    if temp is None:
        temp, _ = _temp_for(lib().nvbio_fastq_temp_bytes, nb, params.max_records, device=dev)
    summary = torch.empty(len(FASTQ_SUMMARY_FIELDS), dtype=torch.int32, device=dev)
    _check(lib().nvbio_fastq_scan(FMIndex._dev_index(dev), _ptr(text) if text.numel() else None, nb, ctypes.byref(params),
                                  ctypes.cast(summary.data_ptr(), ctypes.POINTER(_FastqSummary)), _ptr(temp), temp.numel(), _stream_ptr(dev)))
    return summary, temp


def fastq_encode(text, params, temp, reads4, read_index, quals, names, name_index, status, reads4_capacity_words=None, names_capacity=None,
                 text_bytes=None):
    """nvbio_fastq_encode into caller tensors (reads4 int32 words, quals / names uint8, the indices int32, status: an int32 device word);
    the capacities default to the tensors' sizes.  No synchronisation."""
    dev = text.device
    nb = text.numel() if text_bytes is None else int(text_bytes)
    words = reads4.numel() if reads4_capacity_words is None else int(reads4_capacity_words)
    name_cap = names.numel() if names_capacity is None else int(names_capacity)
    p = lambda t: _ptr(t) if t is not None and t.numel() else None
    _check(lib().nvbio_fastq_encode(FMIndex._dev_index(dev), p(text), nb, ctypes.byref(params), _ptr(temp), temp.numel(), p(reads4), words,
                                    _ptr(read_index), p(quals), p(names), name_cap, _ptr(name_index), _ptr(status), _stream_ptr(dev)))


def fastq_summary(summary):
    """the summary tensor of fastq_scan -> dict (one copy to the host)"""
    return dict(zip(FASTQ_SUMMARY_FIELDS, (int(v) for v in summary.cpu().numpy().view(np.uint32))))


class FastqBatch:
    """The reads of one parsed FASTQ text in HBM, io::SequenceData<DNA_N>-shaped: reads4 (int32 words, 4-bit big-endian), read_index
    (int32 [n + 1], the sequence index), quals (uint8, one per symbol, converted to Phred), names_data (uint8) with name_index (int32
    [n + 1]); summary: the nvbio_fastq_summary as a dict, its fields also attributes (n_records, consumed_bytes, status, ...)."""

    def __init__(self, reads4, read_index, quals, names_data, name_index, summary, device):
        self.reads4, self.read_index, self.quals, self.names_data, self.name_index = reads4, read_index, quals, names_data, name_index
        self.summary, self.device = summary, device
        self.n = summary["n_records"]

    def __getattr__(self, key):
        if key != "summary" and key in self.summary:
            return self.summary[key]
        raise AttributeError(key)

    @property
    def names(self):
        """the (names_data, name_index, max_name_len) triple SamRecords takes as `names`"""
        return self.names_data, self.name_index, self.summary["max_name_len"]

    def read_batch(self):
        """a pipeline.ReadBatch over these arrays: offsets=None when every read has the same length, the int32 read_index otherwise
        (one host synchronisation)"""
        from .pipeline import ReadBatch
        lens = self.read_index[1:] - self.read_index[:-1]
        uniform = self.n == 0 or bool((lens == lens[0]).all().item())
        return ReadBatch(self.reads4, self.n, self.summary["max_read_len"], quals=self.quals, offsets=None if uniform else self.read_index)


def parse_fastq(text, quality_encoding=FASTQ_PHRED33, strand_op=FASTQ_NO_OP, truncate_len=FASTQ_UNLIMITED, max_records=FASTQ_UNLIMITED,
                device="cuda:0"):
    """The bytes of a FASTQ file (bytes, a numpy array or a uint8 device tensor, below 4 GiB) -> FastqBatch: SequenceDataFile_FASTQ_parser
    ::nextChunk and SequenceDataEncoder::push_back (nvbio/io/sequence/sequence_fastq.cpp:39-203, sequence_encoder.cpp:304-368) on the
    device -- the grammar and its departures are in include/nvbio_amd.h ("FASTQ input").  The summary is read once, the arrays are then
    allocated to size.  The scan's temp takes 20 bytes per POSSIBLE record: min(max_records, len(text) / 5); a caller that knows how many
    records a chunk can hold passes max_records.  Errors are reported, not raised: batch.status (FASTQ_STATUS_*), batch.consumed_bytes."""
    torch = _torch()
    t = _fastq_text(text, device)
    params = _FastqParams(int(quality_encoding), int(strand_op), int(truncate_len), int(max_records))
    summary_dev, temp = fastq_scan(t, params)
    s = fastq_summary(summary_dev)
    n = s["n_records"]
    reads4 = torch.empty((s["n_symbols"] + 7) // 8, dtype=torch.int32, device=t.device)
    quals = torch.empty(s["n_symbols"], dtype=torch.uint8, device=t.device)
    names = torch.empty(s["n_name_bytes"], dtype=torch.uint8, device=t.device)
    read_index = torch.empty(n + 1, dtype=torch.int32, device=t.device)
    name_index = torch.empty(n + 1, dtype=torch.int32, device=t.device)
    fastq_encode(t, params, temp, reads4, read_index, quals, names, name_index, summary_dev[6:7])
    s["status"] = int(summary_dev[6].item()) & 0xFFFFFFFF
    if s["status"] & FASTQ_STATUS_CAPACITY:
        raise NvbioError(1, "nvbio_fastq_encode: a record did not fit arrays allocated from the summary")
    return FastqBatch(reads4, read_index, quals, names, name_index, s, t.device)


def read_fastq(path, chunk_bytes=64 << 20, **kw):
    """A generator of FastqBatch over the file at `path`, read in chunks of chunk_bytes: the bytes a chunk's parse did not consume
    (consumed_bytes: the record the chunk cuts) go in front of the next.  A chunk that holds no whole record grows until it does.  At the
    end of the file an unfinished record is the reference's "incomplete read": NvbioError, as is a marker error anywhere.  kw: parse_fastq's."""
    tail, eof, capped = b"", False, False
    with open(path, "rb") as f:
        while True:
            data = b"" if eof or capped else f.read(chunk_bytes)                  # capped: whole records may be left in the tail; parse them first
            eof = eof or (not capped and len(data) < chunk_bytes)
            text = tail + data
            if not text:
                return
            batch = parse_fastq(text, **kw)
            if batch.status & FASTQ_STATUS_MARKER:
                raise NvbioError(1, "%s: FASTQ parse error: byte %d where a record must begin with '@'" % (path, batch.error_char))
            tail = text[batch.consumed_bytes:]
            capped = batch.n > 0 and batch.n == kw.get("max_records", FASTQ_UNLIMITED) and len(tail) > 0
            if batch.n:
                yield batch
            elif eof:
                if batch.status & FASTQ_STATUS_INCOMPLETE:
                    raise NvbioError(1, "%s: incomplete read at the end of the file" % path)
                return


# ---- FASTA input -----------------------------------------------------------------------------------------------------------------
FASTA_PRE, FASTA_ID, FASTA_REST, FASTA_BODY, FASTA_END = 0, 1, 2, 3, 4
FASTA_NO_SYMBOL = 0x100
FASTA_STATUS_INCOMPLETE, FASTA_STATUS_END_BYTE, FASTA_STATUS_OVERFLOW_32, FASTA_STATUS_CAPACITY = 1, 2, 4, 8
FASTA_STATE_FIELDS = ("machine", "n_symbols", "n_seqs", "n_ambs", "n_holes", "n_name_bytes", "last_symbol", "seed")
FASTA_SUMMARY_FIELDS = ("n_symbols", "n_seqs", "n_ambs", "n_holes", "n_name_bytes", "consumed_bytes", "machine", "status")


class _FastaState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in FASTA_STATE_FIELDS] + [("freq", ctypes.c_uint32 * 4), ("max_name_len", ctypes.c_uint32),
                                                                     ("reserved", ctypes.c_uint32 * 3)]


class _FastaSummary(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in FASTA_SUMMARY_FIELDS]


def fasta_state_init(seed=11, device="cuda:0"):
    """nvbio_fasta_state_init -> the state as an int32 device tensor [16]: the carry from chunk to chunk"""
    state = _torch().empty(16, dtype=_torch().int32, device=device)
    _check(lib().nvbio_fasta_state_init(FMIndex._dev_index(device), ctypes.cast(state.data_ptr(), ctypes.POINTER(_FastaState)), int(seed), _stream_ptr(device)))
    return state


def fasta_state(state):
    """the state tensor -> dict (one copy to the host): FASTA_STATE_FIELDS, freq (list of 4), max_name_len"""
    v = [int(x) for x in state.cpu().numpy().view(np.uint32)]
    return dict(zip(FASTA_STATE_FIELDS, v[:8]), freq=v[8:12], max_name_len=v[12])


def fasta_scan(text, state, temp=None, text_bytes=None):
    """nvbio_fasta_scan over a uint8 device tensor entered in `state` (not changed) -> (summary: int32 tensor [8] on the device,
    FASTA_SUMMARY_FIELDS; temp: what fasta_encode reads).  No synchronisation."""
    torch = _torch()
    dev = text.device
    nb = text.numel() if text_bytes is None else int(text_bytes)
    if temp is None:
        temp, _ = _temp_for(lib().nvbio_fasta_temp_bytes, nb, device=dev)
    summary = torch.empty(len(FASTA_SUMMARY_FIELDS), dtype=torch.int32, device=dev)
    _check(lib().nvbio_fasta_scan(FMIndex._dev_index(dev), _ptr(text) if text.numel() else None, nb, ctypes.cast(state.data_ptr(), ctypes.POINTER(_FastaState)),
                                  ctypes.cast(summary.data_ptr(), ctypes.POINTER(_FastaSummary)), _ptr(temp), temp.numel(), _stream_ptr(dev)))
    return summary, temp


def fasta_summary(summary):
    """the summary tensor of fasta_scan -> dict (one copy to the host)"""
    return dict(zip(FASTA_SUMMARY_FIELDS, (int(v) for v in summary.cpu().numpy().view(np.uint32))))


def fasta_encode(text, temp, state, status, text2=None, seq_offset=None, name_index=None, names=None, hole_offset=None, hole_rank=None, hole_amb=None,
                 text2_capacity_words=None, max_seqs=None, names_capacity=None, max_holes=None, text_bytes=None):
    """nvbio_fasta_encode into caller tensors (text2 int32 words; seq_offset / name_index int32 with one entry more than max_seqs; names
    and hole_amb uint8; hole_offset / hole_rank int32; status: an int32 device word); a tensor left None is not written; the capacities
    default to the tensors' sizes.  Advances `state`.  No synchronisation."""
    dev = text.device
    nb = text.numel() if text_bytes is None else int(text_bytes)
    size = lambda t, less=0: 0 if t is None else max(t.numel() - less, 0)
    words = size(text2) if text2_capacity_words is None else int(text2_capacity_words)
    seqs = min(size(seq_offset, 1) if seq_offset is not None else 1 << 32, size(name_index, 1) if name_index is not None else 1 << 32) if max_seqs is None else int(max_seqs)
    holes = min([size(t) for t in (hole_offset, hole_rank, hole_amb) if t is not None] or [0]) if max_holes is None else int(max_holes)
    p = lambda t: _ptr(t) if t is not None and t.numel() else None
    _check(lib().nvbio_fasta_encode(FMIndex._dev_index(dev), p(text), nb, _ptr(temp), temp.numel(), ctypes.cast(state.data_ptr(), ctypes.POINTER(_FastaState)),
                                    p(text2), words, p(seq_offset), p(name_index), seqs if seqs < (1 << 32) else 0, p(names),
                                    size(names) if names_capacity is None else int(names_capacity), p(hole_offset), p(hole_rank), p(hole_amb), holes,
                                    _ptr(status), _stream_ptr(dev)))


def fasta_finish(state, seq_offset=None, name_index=None, hole_offset=None, hole_rank=None, hole_len=None, seq_n_ambs=None, max_seqs=None, max_holes=None):
    """nvbio_fasta_finish: closes the tables behind the last chunk (entry n_seqs of both indices, the holes' lengths, n_ambs per sequence,
    state.max_name_len).  No synchronisation."""
    dev = state.device
    seqs = (min(t.numel() for t in (seq_offset, name_index) if t is not None) - 1 if (seq_offset is not None or name_index is not None) else 0) \
        if max_seqs is None else int(max_seqs)
    holes = (min(t.numel() for t in (hole_offset, hole_rank) if t is not None) if (hole_offset is not None or hole_rank is not None) else 0) \
        if max_holes is None else int(max_holes)
    p = lambda t: _ptr(t) if t is not None and t.numel() else None
    _check(lib().nvbio_fasta_finish(FMIndex._dev_index(dev), ctypes.cast(state.data_ptr(), ctypes.POINTER(_FastaState)), p(seq_offset), p(name_index), max(seqs, 0),
                                    p(hole_offset), p(hole_rank), holes, p(hole_len), p(seq_n_ambs), _stream_ptr(dev)))


class FastaReference:
    """A parsed reference in HBM: text2 (int32 words, 2-bit big-endian: what FMIndex.build and the aligners take as the genome) and length;
    sequence_index (int32 [n + 1]: where each sequence starts), names_data (uint8) with name_index (int32 [n + 1]); the holes -- runs of
    one ambiguous byte, stored as draws -- as hole_offset, hole_len (int32) and hole_amb (uint8); seq_n_ambs (int32 [n]: holes that start
    in each sequence); freq (the counts of the four stored symbols); state: the final nvbio_fasta_state as a dict; status (FASTA_STATUS_*
    of the last chunk: INCOMPLETE means the input ended inside a header line)."""

    def __init__(self, text2, sequence_index, names_data, name_index, hole_offset, hole_len, hole_amb, seq_n_ambs, state, status, device):
        self.text2, self.sequence_index, self.names_data, self.name_index = text2, sequence_index, names_data, name_index
        self.hole_offset, self.hole_len, self.hole_amb, self.seq_n_ambs = hole_offset, hole_len, hole_amb, seq_n_ambs
        self.state, self.status, self.device = state, status, device
        self.length, self.n_seqs, self.n_holes, self.freq, self.seed = state["n_symbols"], state["n_seqs"], state["n_holes"], state["freq"], state["seed"]
        self._names = None

    @property
    def names(self):
        """the sequence names as a list of bytes (one copy to the host, kept)"""
        if self._names is None:
            b, idx = self.names_data.cpu().numpy().tobytes(), u32(self.name_index)
            self._names = [b[idx[i]:idx[i + 1]] for i in range(self.n_seqs)]
        return self._names

    @property
    def holes(self):
        """(offset, len, amb) as three numpy arrays: the BNTAmb table"""
        return u32(self.hole_offset), u32(self.hole_len), self.hole_amb.cpu().numpy()

    def sam_refs(self):
        return SamRefs(self.names, u32(self.sequence_index).astype(np.int64), device=self.device)

    def build_index(self, **build_opts):
        """FMIndex.build over the text (kw: kmer_len, sa_int, table_flags, ...)"""
        return FMIndex.build(self.text2, self.length, device=self.device, **build_opts)

    def save(self, prefix):
        """prefix.pac, prefix.ann and prefix.amb, byte for byte as nvBWT writes them (save_bpac, nvBWT/nvBWT.cu:243-287: 4 symbols a byte,
        a 0 byte when length % 4 == 0, then the byte length % 4; save_bns, nvbio/basic/bnt.cpp:28-73: gi 0, anno "null", a name printed up
        to its first NUL)"""
        n = self.length
        words = u32(self.text2)[:(n + 15) // 16]
        pac = words.astype(">u4").tobytes()[:(n + 3) // 4] + (b"\0" if n % 4 == 0 else b"") + bytes([n % 4])
        off, n_ambs = u32(self.sequence_index), u32(self.seq_n_ambs)
        ann = [b"%d %d %d\n" % (n, self.n_seqs, self.seed)]
        for i, name in enumerate(self.names):
            ann.append(b"0 " + name.split(b"\0")[0] + b" null\n%d %d %d\n" % (off[i], off[i + 1] - off[i], n_ambs[i]))
        amb = [b"%d %d %d\n" % (n, self.n_seqs, self.n_holes)]
        amb += [b"%d %d " % (o, l) + bytes([a]) + b"\n" for o, l, a in zip(*self.holes)]
        for ext, data in (("pac", pac), ("ann", b"".join(ann)), ("amb", b"".join(amb))):
            with open(prefix + "." + ext, "wb") as f:
                f.write(data)


def _fasta_chunks(chunks, total_bytes, seed, device):
    """an iterable of byte chunks through one state -> FastaReference.  text2 is sized from total_bytes (symbols <= bytes); the sequence,
    name and hole arrays grow when a chunk's summary says so: one read of the summary per chunk."""
    torch = _torch()
    dev = torch.device(device)
    state = fasta_state_init(seed, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
    text2 = i32((total_bytes + 15) // 16 + 4)
    arr = dict(seq_offset=i32(65), name_index=i32(65), names=u8(1024), hole_offset=i32(64), hole_rank=i32(64), hole_amb=u8(64))
    n_seqs = n_holes = n_names = 0
    last = 0

    def grow(keys, used, need):
        size = arr[keys[0]].numel()
        if need <= size:
            return
        for k in keys:
            t = torch.empty(max(need, 2 * size), dtype=arr[k].dtype, device=dev)
            t[:used] = arr[k][:used]
            arr[k] = t

    for chunk in chunks:
        t = _fastq_text(chunk, dev)
        summary_dev, temp = fasta_scan(t, state)
        s = fasta_summary(summary_dev)
        if s["status"] & FASTA_STATUS_OVERFLOW_32:
            raise NvbioError(4, "FASTA input: the symbols or name bytes reach 2^32: coordinates are 32-bit")
        grow(("seq_offset", "name_index"), n_seqs, n_seqs + s["n_seqs"] + 1)
        grow(("names",), n_names, n_names + s["n_name_bytes"])
        grow(("hole_offset", "hole_rank", "hole_amb"), n_holes, n_holes + s["n_holes"])
        fasta_encode(t, temp, state, status, text2=text2, **arr)
        n_seqs, n_holes, n_names, last = n_seqs + s["n_seqs"], n_holes + s["n_holes"], n_names + s["n_name_bytes"], s["status"]
        if s["status"] & FASTA_STATUS_END_BYTE:
            break
    hole_len, seq_n_ambs = i32(max(n_holes, 1)), i32(max(n_seqs, 1))
    fasta_finish(state, arr["seq_offset"], arr["name_index"], arr["hole_offset"], arr["hole_rank"], hole_len, seq_n_ambs)
    st = fasta_state(state)
    if int(status.item()) & FASTA_STATUS_CAPACITY:
        raise NvbioError(1, "nvbio_fasta_encode: an item did not fit arrays sized from the summaries")
    return FastaReference(text2[:(st["n_symbols"] + 15) // 16], arr["seq_offset"][:n_seqs + 1], arr["names"][:n_names], arr["name_index"][:n_seqs + 1],
                          arr["hole_offset"][:n_holes], hole_len[:n_holes], arr["hole_amb"][:n_holes], seq_n_ambs[:n_seqs], st, last, dev)


def parse_fasta(text, seed=11, device="cuda:0"):
    """The bytes of a reference FASTA file (bytes, a numpy array or a uint8 device tensor, below 4 GiB) -> FastaReference:
    FASTA_inc_reader::read and nvBWT's Writer (nvbio/fasta/fasta_inl.h:64-122, nvBWT/nvBWT.cu:102-195) on the device -- the grammar and its
    departures are in include/nvbio_amd.h ("FASTA input")."""
    n = text.numel() if hasattr(text, "numel") else len(text)
    return _fasta_chunks([text], n, seed, device)


def read_fasta(paths, chunk_bytes=64 << 20, seed=11, device="cuda:0"):
    """One path or a list of paths, read in order in chunks of chunk_bytes through ONE state (a chunk may end anywhere: in a name, a hole,
    a word) -> FastaReference.  Input that ends inside a header line is an NvbioError."""
    paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)

    def chunks():
        for path in paths:
            with open(path, "rb") as f:
                while True:
                    data = f.read(chunk_bytes)
                    if not data:
                        break
                    yield data

    ref = _fasta_chunks(chunks(), sum(os.path.getsize(p) for p in paths), seed, device)
    if ref.status & FASTA_STATUS_INCOMPLETE:
        raise NvbioError(1, "%s: the input ends inside a header line" % paths[-1])
    return ref


# ---- the mirrors of the headers' structs: C name -> class (abi.bind types a pointer to one as POINTER(mirror); pipeline.py adds its own) -------
_MIRRORS = {
    "nvbio_sam_refs": _SamRefs, "nvbio_sam_records": _SamRecords, "nvbio_fastq_params": _FastqParams, "nvbio_fastq_summary": _FastqSummary,
    "nvbio_fasta_state": _FastaState, "nvbio_fasta_summary": _FastaSummary,
    "nvbio_fm_index_view": _View, "nvbio_fm_build_options": _BuildOptions, "nvbio_string_set": _StringSet, "nvbio_rank_dictionary": _RankDict,
    "nvbio_mem_params": _MemParams, "nvbio_qgram_index_view": _QGramView, "nvbio_qgroup_index_view": _QGroupView,
    "nvbio_sufsort_stats": _SufsortStats, "nvbio_hit_queues": _HitQueues, "nvbio_seed_hits_params": _SeedHitsParams,
    "nvbio_ragged_seed_layout": _RaggedSeedLayout, "nvbio_all_hits_params": _AllHitsParams, "nvbio_pe_params": _PeParams,
    "nvbio_pe_ragged": _PeRagged, "nvbio_gotoh_scheme": _Scheme, "nvbio_sw_scheme": _SWScheme, "nvbio_alignment_batch": _Batch,
    "nvbio_mapq_params": _MapqParams,
    "nvbio_host_all_mapping_params": _AllMappingParams, "nvbio_host_all_mapping_output": _AllMappingOutput,
    "nvbio_host_all_mapping_stats": _AllMappingStats,
}
