"""The seed locus lines on the GPU: the builder against the brute-force meaning of the uniqueness plane, the two-strand seed pass with the
locus path on and off against the per-strand operators (the oracle, through the helpers of test_gpu_seed_pass.py), the routes the path
really takes against a CPU prediction, and the pipeline end to end with the path on and off.

The builder's rule, as tested here: u[x] = 1 iff text[x, x + len) occurs once over both strands AND neither its last k symbols nor its
first k symbols form a k-mer with more than 8 occurrences (test_seed_locus_layout.table_unique).  The second k-mer is the one a lane on
the reverse strand looks up; without it such a lane could skip a gather that would have sent it to the ordinary search."""
import importlib

import numpy as np
import pytest

from test_gpu_seed_pass import _expected, _tile_major
from test_seed_locus_layout import brute_unique, locus_lines, occurrences, table_unique, window_codes

pytestmark = pytest.mark.gpu


def _rc(a):
    a = np.asarray(a)
    return np.where(a[..., ::-1] < 4, 3 - a[..., ::-1], 4).astype(np.uint8)


def _lines_of(amd, fmi, n, seed_len):
    import torch
    out = torch.zeros(amd.seed_locus_bytes(n), dtype=torch.uint8, device="cuda")
    out.fill_(0xA5)                                                             # the builder owns every byte
    fmi.build_seed_locus(seed_len, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64).reshape(-1, 16)


def _builder_text(rng, n, length):
    text = rng.integers(0, 4, n, dtype=np.uint8)
    text[200:300] = np.tile(np.array([0, 1], dtype=np.uint8), 50)              # a tandem repeat
    el3, el12 = text[400:460].copy(), text[500:560].copy()                      # a planted 60-symbol element: 3 copies, and 12 (heavy k-mers)
    for c in range(1, 3):
        text[2000 + 90 * c:2060 + 90 * c] = el3
    for c in range(1, 12):
        text[700 + 80 * c:760 + 80 * c] = el12
    text[1700:1780] = _rc(text[20:100])                                         # a reverse-complement copy
    half = text[1800:1800 + length // 2].copy()
    text[1800 + length // 2:1800 + length] = _rc(half)                          # a window that is its own reverse complement
    text[1900:1940] = 2                                                         # a homopolymer run
    return text


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k", [5, 9, 15])
def test_builder_against_the_brute_force(amd, orc, k, wide):
    import torch
    rng = np.random.default_rng(1400 + k)
    length = k + 5
    n_unique = 0
    for n_mod in (0, 1, 63, 64, 127):
        n = 2944 + n_mod                                                        # 2944 = 23 * 128
        text = _builder_text(rng, n, length)
        fmi = amd.FMIndex.build(orc.pack2(text), n, kmer_len=k, sa_int=1, table_flags=amd.FM_TABLE_CANONICAL_WIDE if wide else amd.FM_TABLE_CANONICAL)
        lines = _lines_of(amd, fmi, n, length)
        brute, want = brute_unique(text, length), table_unique(text, length, k)
        light = occurrences(text, k) <= 8
        assert lines.shape == ((n >> 7) + 1, 16)
        u = np.zeros(n, dtype=np.uint8)
        for x in range(n):                                                      # u as line x >> 7 holds it
            u[x] = (int(lines[x >> 7, 3 * ((x & 127) >> 6) + 2]) >> (x & 63)) & 1
        assert (u <= brute).all(), (k, wide, n)
        m = n - length + 1
        both_light = np.zeros(n, dtype=bool); both_light[:m] = light[:m] & light[length - k:length - k + m]
        assert np.array_equal(u[both_light], brute[both_light]), (k, wide, n)
        assert not u[~both_light].any() and not u[m:].any()
        # the self-complementary window, the repeats and the reverse-complement copy are off
        assert u[1800] == 0 and not u[400:430].any() and not u[1700:1750].any() and not u[20:70].any()
        # planes equal to the text, u in every line that holds it, pad words and every bit at or beyond n zero: the whole array
        assert np.array_equal(lines, locus_lines(text, want)), (k, wide, n)
        n_unique += int(u.sum())
        if n_mod == 1:
            # a misaligned buffer is refused; so is a seed length the table does not serve
            buf = torch.zeros(amd.seed_locus_bytes(n) + 128, dtype=torch.uint8, device="cuda")
            with pytest.raises(amd.NvbioError):
                fmi.build_seed_locus(length, out=buf[8:8 + amd.seed_locus_bytes(n)])
            with pytest.raises(amd.NvbioError):
                fmi.build_seed_locus(k + 8)
            # the handle's own lines: built for 22 where the table serves 22, rebuilt on request
            own = fmi.seed_locus()
            assert (own is not None and own[1] == 22) if k == 15 else own is None
            before = fmi.device_bytes()
            fmi.build_seed_locus(length)
            assert fmi.seed_locus()[1] == length
            assert fmi.device_bytes() == before + (0 if k == 15 else amd.seed_locus_bytes(n))
        fmi.close()
    assert n_unique > (3000 if k > 5 else 0)


# ---- the pass ----------------------------------------------------------------------------------------------------------------------
N_TEXT = 100003


def _world_text(rng):
    text = rng.integers(0, 4, N_TEXT, dtype=np.uint8)
    unit = rng.integers(0, 4, 300, dtype=np.uint8)
    for c in range(12):                                                         # a 12-copy family: heavy k-mers, residual seeds
        text[30000 + 1000 * c:30300 + 1000 * c] = unit
    for c in range(3):                                                          # a 3-copy family: groups, several hits
        text[50000 + 700 * c:50200 + 700 * c] = text[1000:1200]
    text[55000:55200] = text[2000:2200]                                         # a 2-copy element: an anchor with two hits
    text[60000:60300] = _rc(text[5000:5300])                                    # a reverse-complement copy
    for length, at in ((22, 70000), (14, 71000)):                               # windows that are their own reverse complement
        text[at + length // 2:at + length] = _rc(text[at:at + length // 2])
    return text


@pytest.fixture(scope="module")
def world(amd, orc):
    rng = np.random.default_rng(1414)
    text = _world_text(rng)
    w = dict(text=text, hidx=orc.build_index(text), fmi={}, u={})
    for k, length in ((15, 22), (9, 14)):
        fmi = amd.FMIndex.build(orc.pack2(text), N_TEXT, kmer_len=k, sa_int=1, table_flags=amd.FM_TABLE_CANONICAL_WIDE if k == 15 else amd.FM_TABLE_CANONICAL)
        if k == 9:
            assert fmi.seed_locus() is None
            fmi.build_seed_locus(length)
        assert fmi.seed_locus()[1] == length
        w["fmi"][k] = fmi
        w["u"][k] = table_unique(text, length, k)
    yield w
    for fmi in w["fmi"].values():
        fmi.close()


def _take(text, starts, M):
    return np.stack([text[s:s + M] for s in starts]).copy()


def _mix_strands(rng, reads):
    rcm = rng.random(len(reads)) < 0.5
    reads[rcm] = _rc(reads[rcm])
    return reads


def _case_reads(name, rng, text, M, L, S):
    """one small batch per case; R is never a multiple of the reads per tile, so the last tile is partial"""
    n = len(text)
    R = 203
    free = lambda R: rng.integers(3000, 29000 - M, R)                           # text without planted copies
    if name == "clean":
        return _mix_strands(rng, _take(text, free(R), M))
    if name == "sub_in_anchor":
        reads = _take(text, free(R), M)
        at = rng.integers(0, L, R)
        reads[np.arange(R), at] = (reads[np.arange(R), at] + 1 + rng.integers(0, 3, R)) % 4
        return _mix_strands(rng, reads)
    if name == "sub_in_other":
        reads = _take(text, free(R), M)
        at = rng.integers(L, M, R)
        reads[np.arange(R), at] = (reads[np.arange(R), at] + 1 + rng.integers(0, 3, R)) % 4
        return _mix_strands(rng, reads)
    if name == "indel":
        out = []
        for s in free(R):
            d, at = int(rng.integers(1, 4)), int(rng.integers(L, M - L))
            if rng.random() < 0.5:                                              # a deletion from the read
                out.append(np.concatenate([text[s:s + at], text[s + at + d:s + M + d]]))
            else:                                                               # an insertion into it
                out.append(np.concatenate([text[s:s + at], rng.integers(0, 4, d, dtype=np.uint8), text[s + at:s + M - d]]))
        return _mix_strands(rng, np.stack(out))
    if name == "overhang":
        out = []
        for i in range(R):
            h = int(rng.integers(1, M - L))
            junk = rng.integers(0, 4, h, dtype=np.uint8)
            end = np.concatenate([text[n - M + h:], junk])                      # hangs over the text's end: forward lanes leave [0, n - len]
            start = np.concatenate([junk, text[:M - h]])                        # hangs over its start: reverse lanes do
            out.append((end, _rc(end), start, _rc(start))[i % 4])
        return np.stack(out)
    if name == "repeats":
        starts = np.concatenate([30000 + 1000 * rng.integers(0, 12, 80) + rng.integers(-60, 280, 80),
                                 50000 + 700 * rng.integers(0, 3, 80) + rng.integers(-60, 180, 80),
                                 60000 + rng.integers(-60, 280, R - 160)])
        return _mix_strands(rng, _take(text, starts, M))
    if name == "anchor_two_hits":
        starts = np.where(rng.random(R) < 0.5, 2000, 55000) + rng.integers(0, 200 - L, R)       # the anchor lies in the 2-copy element
        return _mix_strands(rng, _take(text, starts, M))
    if name == "n_in_anchor":
        reads = _take(text, free(R), M)
        reads[np.arange(R), rng.integers(0, L, R)] = 4
        return _mix_strands(rng, reads)
    if name == "n_in_other":
        reads = _take(text, free(R), M)
        reads[np.arange(R), rng.integers(L, M, R)] = 4
        return _mix_strands(rng, reads)
    if name == "self_complementary":
        at = 70000 if L == 22 else 71000
        spr = (M - L) // S + 1
        starts = at - S * rng.integers(0, spr, R) + np.where(rng.random(R) < 0.3, rng.integers(-3, 4, R), 0)     # a seed that IS the window
        return _mix_strands(rng, _take(text, starts, M))
    raise KeyError(name)


def _run(amd, fmi, qs, M, flags=0, inline_hits=0, defer=False, grid_blocks=0):
    b = fmi.match_seed_diagonals_both(qs, M, flags=flags, inline_hits=inline_hits, defer_heavy=defer, grid_blocks=grid_blocks)
    c = [int(v) for v in b["counts"][:4].cpu().numpy()]
    keys = b["keys"][:c[0]].cpu().numpy()
    nq = qs.n
    res = []
    for lo, cnt in ((0, c[1]), (nq, c[2])):
        rr = amd.u32(b["ranges"][lo:lo + cnt]); ids = b["ids"][lo:lo + cnt].cpu().numpy()
        res.append({int(i): (int(a), int(d)) for i, (a, d) in zip(ids, rr)})
    out = dict(keys=keys, in_tiles=c[3], res=res, tile_offsets=b["tile_offsets"].cpu().numpy().copy())
    if flags & amd.FM_COUNT_SECTORS:
        out["sectors"] = int(b["counts"][4:6].cpu().numpy().view(np.uint64)[0])
        out["routes"] = [int(v) for v in b["counts"][6:10].cpu().numpy()]
    return out


def _same(a, b, what):
    """two runs left the same: the tiles' keys key for key, the tile spans, the residual lists, and behind the tiles the deferred
    searches' keys (appended workgroup by workgroup: as a set)"""
    assert a["in_tiles"] == b["in_tiles"], what
    assert np.array_equal(a["keys"][:a["in_tiles"]], b["keys"][:b["in_tiles"]]), what
    assert np.array_equal(np.sort(a["keys"][a["in_tiles"]:]), np.sort(b["keys"][b["in_tiles"]:])), what
    assert np.array_equal(a["tile_offsets"], b["tile_offsets"]), what
    assert a["res"] == b["res"], what


def _check_uniform(amd, orc, world, k, reads, M, L, S, what, expect_path=None):
    fmi, hidx = world["fmi"][k], world["hidx"]
    R = reads.shape[0]
    spr = (M - L) // S + 1
    qs = amd.PackedStringSet(orc.pack4(reads.reshape(-1)), 4, R * spr, fixed_len=L, stride=M, seeds_per_string=spr, seed_interval=S)
    want_f, res_f = _expected(orc, hidx, reads, M, L, S, 0)
    want_r, res_r = _expected(orc, hidx, reads, M, L, S, 1)
    want = _tile_major(want_f, want_r, spr)
    on, off = _run(amd, fmi, qs, M), _run(amd, fmi, qs, M, flags=amd.FM_NO_SEED_LOCUS)
    for got, tag in ((on, "on"), (off, "off")):
        assert np.array_equal(got["keys"], want), (what, tag)
        assert got["res"] == [res_f, res_r], (what, tag)
    _same(on, off, what)
    cnt = _run(amd, fmi, qs, M, flags=amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS)
    _same(cnt, off, (what, "count"))
    if expect_path is not None:
        assert (cnt["routes"][1] > 0) == expect_path, (what, cnt["routes"])
    for h, defer, gb in ((4, False, 0), (1, True, 0), (4, True, 64)):
        a = _run(amd, fmi, qs, M, inline_hits=h, defer=defer, grid_blocks=gb)
        b = _run(amd, fmi, qs, M, inline_hits=h, defer=defer, grid_blocks=gb, flags=amd.FM_NO_SEED_LOCUS)
        _same(a, b, (what, h, defer, gb))
    return cnt


CASES = ["clean", "sub_in_anchor", "sub_in_other", "indel", "overhang", "repeats", "anchor_two_hits", "n_in_anchor", "n_in_other", "self_complementary"]


@pytest.mark.parametrize("k", [9, 15])
@pytest.mark.parametrize("case", CASES)
def test_pass_with_the_path_on_and_off(amd, orc, world, case, k):
    rng = np.random.default_rng(7000 + 31 * CASES.index(case) + k)
    L = 22 if k == 15 else 14
    M, S = 100, 10
    reads = _case_reads(case, rng, world["text"], M, L, S)
    _check_uniform(amd, orc, world, k, reads, M, L, S, (case, k))


GEOMETRIES = {"len193": (193, 0, 10), "len194": (194, 0, 10), "spr1": (0, 0, 1), "spr2": (0, 18, 18), "spr9": (0, 128, 16), "spr64": (0, 63, 1)}


@pytest.mark.parametrize("k", [9, 15])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_pass_read_lengths_and_seed_geometries(amd, orc, world, geom, k):
    """read_len 193 (the longest read one line holds: path on) and 194 (path off, results equal); 1, 2, 9 and 64 seeds per read: tiles
    of 64, 32, 7 and 1 reads"""
    rng = np.random.default_rng(7700 + 13 * list(GEOMETRIES).index(geom) + k)
    L = 22 if k == 15 else 14
    M, extra, S = GEOMETRIES[geom]
    M = M or L + extra
    spr = (M - L) // S + 1
    assert not geom.startswith("spr") or spr == int(geom[3:])
    text = world["text"]
    R = 203 if spr <= 2 else 3 * (64 // spr) + 1                               # the last tile is partial
    reads = _mix_strands(rng, _take(text, rng.integers(0, N_TEXT - M, R), M))
    mut = rng.random(reads.shape) < 0.01
    reads[mut] = (reads[mut] + 1) % 4
    _check_uniform(amd, orc, world, k, reads, M, L, S, (geom, k), expect_path=None if spr == 1 else M <= 193)


@pytest.mark.parametrize("k", [9, 15])
def test_pass_over_ragged_reads(amd, orc, world, k):
    """ragged reads take the same path with their own offsets and lengths; reads longer than 193 symbols among them gather as ever.  The
    path on and off leave the same, defer on and off, in-line hits 1 and 4 (the ragged pass without the path is held against the
    operators by test_gpu_seed_pass.py)."""
    rng = np.random.default_rng(7800 + k)
    L = 22 if k == 15 else 14
    text = world["text"]
    R, Mmax = 301, 230
    lens = rng.integers(40, Mmax + 1, R); lens[:20] = rng.integers(5, L + 2, 20); lens[20:40] = 193; lens[40:60] = 194
    starts = rng.integers(0, N_TEXT - Mmax, R)
    starts[60:120] = 30000 + 1000 * rng.integers(0, 12, 60) + rng.integers(-60, 280, 60)
    full = _take(text, starts, Mmax)
    mut = rng.random(full.shape) < 0.01
    full[mut] = (full[mut] + 1) % 4
    full[rng.random(full.shape) < 0.002] = 4
    rcm = rng.random(R) < 0.5
    flat = np.concatenate([_rc(full[r, :lens[r]]) if rcm[r] else full[r, :lens[r]] for r in range(R)])
    offs = np.zeros(R + 1, dtype=np.int64); offs[1:] = np.cumsum(lens)
    itab = np.maximum((np.float32(1.0) + np.float32(1.15) * np.sqrt(np.arange(Mmax + 1, dtype=np.float32))).astype(np.int32), 1)
    ivs = itab[lens]
    spr = int(np.where(lens >= L, (lens - L) // ivs + 1, 0).max())
    qs = amd.PackedStringSet(orc.pack4(flat), 4, R * spr, offsets=offs.astype(np.uint32), fixed_len=L, stride=0, seeds_per_string=spr,
                             seed_intervals=ivs.astype(np.uint32))
    fmi = world["fmi"][k]
    for h, defer in ((1, False), (4, False), (1, True), (4, True)):
        a = _run(amd, fmi, qs, Mmax, inline_hits=h, defer=defer)
        b = _run(amd, fmi, qs, Mmax, inline_hits=h, defer=defer, flags=amd.FM_NO_SEED_LOCUS)
        _same(a, b, (k, h, defer))
    cnt = _run(amd, fmi, qs, Mmax, flags=amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS)
    assert cnt["routes"][0] > R // 2 and cnt["routes"][1] > R


# ---- the path is really taken --------------------------------------------------------------------------------------------------------
def _predict_routes(text, u, reads, L, S, k, wide, path=True):
    """(routes, lines) the pass must count for N-free reads of one length: reads with a usable anchor, windows settled on the locus, windows
    of such reads that gather, windows of the other reads (the last three over j > 0); lines = the gathered 64-byte sectors with the path"""
    n = len(text)
    R, M = reads.shape
    spr = (M - L) // S + 1
    fw, rc = window_codes(text, L)
    order = np.argsort(fw, kind="stable"); sfw = fw[order]
    kocc = occurrences(text, k)
    kfw, _ = window_codes(text, k)
    kord = np.argsort(kfw, kind="stable"); skf = kfw[kord]
    grp_from = 3 if wide else 2

    def hits(code):
        lo, hi = np.searchsorted(sfw, code, "left"), np.searchsorted(sfw, code, "right")
        return order[lo:hi]

    def kmer_occ(window):                                                       # occurrences over both strands of the window's last k symbols
        c, r = window_codes(window[L - k:], k)
        tot = 0
        for code in (int(c[0]), int(r[0])):
            lo, hi = np.searchsorted(skf, code, "left"), np.searchsorted(skf, code, "right")
            tot += hi - lo
        return tot
    routes, lines = [0, 0, 0, 0], 0
    for rd in reads:
        wins = [rd[j * S:j * S + L] for j in range(spr)]
        codes = [window_codes(w, L) for w in wins]
        occ = [kmer_occ(w) for w in wins]
        f, r = hits(int(codes[0][0][0])), hits(int(codes[0][1][0]))
        usable = path and occ[0] <= 8 and len(f) + len(r) == 1
        assert max(occ) <= 8                                                    # (a heavy k-mer takes the ordinary search: its sectors are not predicted here)
        lines += 1 + (grp_from <= occ[0] <= 8)
        asked = False
        for j in range(1, spr):
            settled = False
            if usable:
                x = int(f[0]) + j * S if len(f) else int(r[0]) - j * S
                if 0 <= x <= n - L:
                    asked = True
                    t = text[x:x + L]
                    settled = bool(u[x]) and np.array_equal(t if len(f) else _rc(t), wins[j])
            routes[1] += settled
            routes[2] += path and usable and not settled
            routes[3] += path and not usable
            if not settled:
                lines += 1 + (grp_from <= occ[j] <= 8)
        routes[0] += usable
        lines += asked
    return routes, lines


@pytest.mark.parametrize("k", [9, 15])
def test_the_path_is_really_taken(amd, orc, world, k):
    rng = np.random.default_rng(7900 + k)
    text, u, fmi = world["text"], world["u"][k], world["fmi"][k]
    L = 22 if k == 15 else 14
    M, S, R = 100, 10, 203
    spr = (M - L) // S + 1
    wide = k == 15
    # error-free reads from unique text: every window of the read has u = 1
    ok = np.nonzero(np.convolve(u[:N_TEXT - M].astype(np.int64) == 0, np.ones(M - L + 1, dtype=np.int64))[M - L:] == 0)[0]
    ok = ok[(ok > 3000) & (ok < 29000 - M)]
    clean = _mix_strands(rng, _take(text, rng.choice(ok, R, replace=False), M))
    batches = {"clean": clean}
    kocc = occurrences(text, k)
    for name in ("sub_in_anchor", "sub_in_other"):
        # (reads without a window whose k-mer has more than 8 occurrences: those take the ordinary search, whose sectors are not predicted)
        reads = _case_reads(name, rng, text, M, L, S)
        kf, kr = window_codes(text, k)
        heavy = set(kf[kocc[:len(kf)] > 8].tolist()) | set(kr[kocc[:len(kf)] > 8].tolist())
        keep = [i for i, rd in enumerate(reads) if not (set(window_codes(rd, k)[0].tolist()) & heavy)]
        # (... nor a window with several hits on one strand: with one in-line hit allowed it takes the ordinary search too)
        lf, lr = window_codes(text, L)
        many = set(v for v, c in zip(*np.unique(lf, return_counts=True)) if c > 1)
        many |= set(v for v, c in zip(*np.unique(lr, return_counts=True)) if c > 1)
        keep = [i for i in keep if not (many & set(c for j in range(spr) for c in (int(window_codes(reads[i][j * S:j * S + L], L)[0][0]), int(window_codes(reads[i][j * S:j * S + L], L)[1][0]))))]
        batches[name] = reads[keep]
    for name, reads in batches.items():
        R = len(reads)
        qs = amd.PackedStringSet(orc.pack4(reads.reshape(-1)), 4, R * spr, fixed_len=L, stride=M, seeds_per_string=spr, seed_interval=S)
        got = _run(amd, fmi, qs, M, flags=amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS)
        routes, lines = _predict_routes(text, u, reads, L, S, k, wide)
        assert got["routes"] == routes, (name, k, got["routes"], routes)
        assert got["sectors"] == lines, (name, k, got["sectors"], lines)
        if name == "clean":
            # every read placed by its anchor, every other window settled on the locus: 2 lines per read plus the anchors' group lines
            # (an anchor whose k-mer has a group brings one more: at most one per read)
            assert routes == [R, R * (spr - 1), 0, 0] and 2 * R <= lines <= 3 * R
            assert got["sectors"] - 2 * R == sum(1 for rd in reads if _predict_routes(text, u, rd[None, :], L, S, k, wide)[1] == 3)
        else:
            assert min(routes[1:] if name == "sub_in_other" else [routes[3]]) > 0
        # without the path: one line per window plus the group lines
        off = _run(amd, fmi, qs, M, flags=amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS | amd.FM_NO_SEED_LOCUS)
        routes_off, lines_off = _predict_routes(text, u, reads, L, S, k, wide, path=False)
        assert off["routes"] == routes_off == [0, 0, 0, 0]
        assert off["sectors"] == lines_off and lines_off >= spr * R, (name, k)
    with pytest.raises(amd.NvbioError):                                         # the route counts go with the sector count only
        fmi.match_seed_diagonals_both(qs, M, flags=amd.FM_COUNT_LOCUS)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_pipeline_with_the_path_on_and_off(amd, orc, world):
    """pipeline.seed_and_extend on the 100 kbp text: the same best and second-best alignments and mapping qualities with the A/B bit on
    and off, from a handle built without the lines and from one whose lines were rebuilt for another seed length"""
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    rng = np.random.default_rng(8000)
    text = world["text"]
    G = N_TEXT
    genome2 = orc.pack2(text)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    R, M = 2000, 100
    starts = rng.integers(0, G - M - 8, R)
    starts[:300] = 30000 + 1000 * rng.integers(0, 12, 300) + rng.integers(0, 200, 300)
    starts[300:500] = 50000 + 700 * rng.integers(0, 3, 200) + rng.integers(0, 100, 200)
    reads = _take(text, starts, M)
    mut = rng.random(reads.shape) < 0.02
    reads[mut] = (reads[mut] + 1 + rng.integers(0, 3, int(mut.sum()))) % 4
    reads = _mix_strands(rng, reads)
    reads[-20:] = rng.integers(0, 4, (20, M))
    rb = pipeline.ReadBatch(torch.from_numpy(orc.pack4(reads.reshape(-1)).view(np.int32)).cuda(), R, M)

    def run(fmi, seed_len, bit):
        params = pipeline.SeedExtendParams.end_to_end()
        params.seed_len = seed_len
        params.mapq = True
        params.algo_flags = (params.algo_flags or 0) | (amd.SEED_NO_LOCUS if bit else 0)
        ex = {}
        bs, bp, brc, nc = pipeline.seed_and_extend(fmi, g_dev, G, rb, params, extras=ex)
        torch.cuda.synchronize()
        return [np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t).copy() for t in (bs, bp, brc, nc, ex["second_score"], ex["second"], ex["mapq"])]

    flags = amd.FM_TABLE_CANONICAL_WIDE
    bare = amd.FMIndex.build(genome2, G, kmer_len=15, sa_int=1, table_flags=flags | amd.FM_TABLE_NO_SEED_LOCUS)
    assert bare.seed_locus() is None
    other = amd.FMIndex.build(genome2, G, kmer_len=15, sa_int=1, table_flags=flags)
    assert other.seed_locus()[1] == 22 and other.device_bytes() == bare.device_bytes() + amd.seed_locus_bytes(G)
    for seed_len in (22, 20):
        want = run(bare, seed_len, False)
        assert len(np.unique(want[0])) > 3 and len(np.unique(want[6])) > 3     # scores and mapping qualities of many kinds
        for fmi in (world["fmi"][15], other):
            for bit in (False, True):
                got = run(fmi, seed_len, bit)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b), (seed_len, bit)
        other.build_seed_locus(20)                                              # the second round: `other` serves 20, the shared handle still 22
        assert other.seed_locus()[1] == 20
    bare.close(); other.close()
