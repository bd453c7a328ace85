"""The schedule of the locus seed pass (csrc/fm_canon_inl.h: fm_seed_locus_loop): its steady state, its fill and drain, the grid and the
seeds per read.

The cases of test_gpu_seed_locus.py are small: most waves there own no tile or one, so a wave hardly ever has every stage of the loop
busy, and the iterations that fill and drain the stages are barely run.  Here `grid_blocks=64` leaves 256 waves, and the batches have
hundreds to thousands of tiles: every wave runs the five stages (words | anchor entries | locus words | remaining entries | groups and
resolution) over several tiles, on reads of every route.  A change of the schedule must leave every key, count, residual and deferred
search as it was: against the path switched off, and against the per-strand operators of the oracle -- for uniform reads and for ragged
ones, which run a kernel form of their own.

Seed lengths: 22 symbols at k = 15 and 14 at k = 9 (the table answers seeds of k .. k + 7 symbols, as in test_gpu_seed_locus.py).
"""
import numpy as np
import pytest

from test_gpu_seed_pass import _expected
from test_seed_locus_layout import window_codes
from test_gpu_seed_locus import CASES, _case_reads, _mix_strands, _rc, _run, _same, _take, _world_text

pytestmark = pytest.mark.gpu

N_BIG = 300007                              # the planted text of test_gpu_seed_locus.py, then random symbols
STAGES = 5                                  # stages of fm_seed_locus_loop
WAVES = 256                                 # grid_blocks = 64
M, S = 150, 16                              # 9 seeds per read: tiles of 7 reads
ROUNDS = 8                                  # x 10 cases x 203 reads = 16240 reads, 2320 tiles, 9 per wave


def _seed_len(k):
    return 22 if k == 15 else 14


def _tile_major(keys_f, keys_r, rpt):
    """the order of the two-strand pass: tile by tile, a tile's forward keys, then its reverse-strand keys (a stable sort)"""
    keys = np.concatenate([keys_f, keys_r])
    return keys[np.argsort(((keys >> 34) // rpt) * 2 + ((keys >> 33) & 1), kind="stable")]


@pytest.fixture(scope="module")
def big(amd, orc):
    """the text, its two handles, and per k one pool of reads of every route with what the operators leave for them -- computed once"""
    rng = np.random.default_rng(1515)
    text = np.concatenate([_world_text(rng), rng.integers(0, 4, N_BIG - 100003, dtype=np.uint8)])
    assert len(text) == N_BIG
    w = dict(text=text, hidx=orc.build_index(text), fmi={}, pool={})
    for k in (15, 9):
        L = _seed_len(k)
        fmi = amd.FMIndex.build(orc.pack2(text), N_BIG, kmer_len=k, sa_int=1, table_flags=amd.FM_TABLE_CANONICAL_WIDE if k == 15 else amd.FM_TABLE_CANONICAL)
        if k == 9:
            fmi.build_seed_locus(L)
        assert fmi.seed_locus()[1] == L
        w["fmi"][k] = fmi
        reads = np.concatenate([_case_reads(c, rng, text, M, L, S) for _ in range(ROUNDS) for c in CASES])
        reads = reads[rng.permutation(len(reads))]
        w["pool"][k] = dict(reads=reads, f=_expected(orc, w["hidx"], reads, M, L, S, 0), r=_expected(orc, w["hidx"], reads, M, L, S, 1))
    yield w
    for fmi in w["fmi"].values():
        fmi.close()


def _uniform_set(amd, orc, reads, L, m=M, s=S):
    R = reads.shape[0]
    spr = (m - L) // s + 1
    return amd.PackedStringSet(orc.pack4(reads.reshape(-1)), 4, R * spr, fixed_len=L, stride=m, seeds_per_string=spr, seed_interval=s)


def _prefix_expected(pool, R, spr):
    """what the operators leave for the pool's first R reads: keys carry their read, residual entries their seed"""
    (kf, rf), (kr, rr) = pool["f"], pool["r"]
    want = _tile_major(kf[(kf >> 34) < R], kr[(kr >> 34) < R], 64 // spr)
    return want, [{i: v for i, v in d.items() if i < R * spr} for d in (rf, rr)]


def _anchors_through_a_group(text, reads, L, k, wide):
    """reads whose first seed is placed -- one hit over both strands -- through a group: the k-mer the table is asked for occurs
    3 .. 8 times (16-byte entries; 2 .. 8 with 8-byte ones), both orientations counted"""
    clean = (reads[:, :L] < 4).all(axis=1)
    anchors = reads[clean, :L]
    def codes(a, length):                                                       # code of every row, of its reverse complement
        t = a.astype(np.int64)
        fw = sum(t[:, i] << (2 * i) for i in range(length))
        rc = sum((3 - t[:, i]) << (2 * (length - 1 - i)) for i in range(length))
        return fw, rc
    def occ(fw, rc, length):
        vals, cnt = np.unique(window_codes(text, length)[0], return_counts=True)
        def count(c):
            i = np.minimum(np.searchsorted(vals, c), len(vals) - 1)
            return np.where(vals[i] == c, cnt[i], 0)
        return count(fw) + count(rc)
    hits = occ(*codes(anchors, L), L)
    kocc = occ(*codes(anchors[:, L - k:], k), k)
    return int(((hits == 1) & (kocc >= (3 if wide else 2)) & (kocc <= 8)).sum())


@pytest.mark.parametrize("k", [9, 15])
def test_steady_state_uniform_reads(amd, orc, big, k):
    """nine tiles per wave of reads of every route: the path on against the path off and the operators; DEFER on and off, in-line hits
    1 and 4; and the batch really holds every route, or it would prove nothing"""
    L, fmi, pool = _seed_len(k), big["fmi"][k], big["pool"][k]
    reads = pool["reads"]
    R, spr = len(reads), (M - L) // S + 1
    assert -(-R // (64 // spr)) >= 9 * WAVES
    qs = _uniform_set(amd, orc, reads, L)
    want, res = _prefix_expected(pool, R, spr)
    on, off = _run(amd, fmi, qs, M, grid_blocks=64), _run(amd, fmi, qs, M, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
    for got, tag in ((on, "on"), (off, "off")):
        assert np.array_equal(got["keys"], want), (k, tag)
        assert got["res"] == res, (k, tag)
    _same(on, off, k)
    deferred = 0
    for h, defer in ((1, False), (4, False), (1, True), (4, True)):
        a = _run(amd, fmi, qs, M, inline_hits=h, defer=defer, grid_blocks=64)
        b = _run(amd, fmi, qs, M, inline_hits=h, defer=defer, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
        _same(a, b, (k, h, defer))
        if defer:
            deferred += len(a["keys"]) - a["in_tiles"]                          # keys appended behind the tiles: searches that were deferred
    cnt = _run(amd, fmi, qs, M, grid_blocks=64, flags=amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS)
    _same(cnt, off, (k, "count"))
    placed, settled, gathered, unplaced = cnt["routes"]
    through_group = _anchors_through_a_group(big["text"], reads, L, k, k == 15)
    print("k", k, "reads", R, "routes", cnt["routes"], "anchors through a group", through_group, "deferred keys", deferred, "lines", cnt["sectors"])
    assert settled > 0 and gathered > 0 and unplaced > 0 and through_group > 0 and deferred > 0
    assert placed + unplaced // (spr - 1) == R


@pytest.mark.parametrize("k", [9, 15])
def test_steady_state_ragged_reads(amd, orc, big, k):
    """the same reads cut to 100 .. 150 symbols, each with its own seed interval -- the kernel form of ragged reads, nine tiles per wave:
    the path on against the path off and against the per-strand operators (read by read what they leave for a uniform batch of that
    read's length); DEFER on and off, in-line hits 1 and 4; and the batch holds every route"""
    rng = np.random.default_rng(1520 + k)
    L, fmi, hidx = _seed_len(k), big["fmi"][k], big["hidx"]
    reads = big["pool"][k]["reads"]
    R = len(reads)
    lens = rng.integers(100, M + 1, R)
    flat = np.concatenate([reads[r, :lens[r]] for r in range(R)])
    offs = np.zeros(R + 1, dtype=np.int64); offs[1:] = np.cumsum(lens)
    itab = np.maximum((np.float32(1.0) + np.float32(1.15) * np.sqrt(np.arange(M + 1, dtype=np.float32))).astype(np.int32), 1)
    ivs = itab[lens]
    nseeds = (lens - L) // ivs + 1
    spr = int(nseeds.max())
    assert -(-R // (64 // spr)) >= 9 * WAVES
    qs = amd.PackedStringSet(orc.pack4(flat), 4, R * spr, offsets=offs.astype(np.uint32), fixed_len=L, stride=0, seeds_per_string=spr,
                             seed_intervals=ivs.astype(np.uint32))
    # the operators, length group by length group
    want_keys, want_res = [[], []], [{}, {}]
    for ln in np.unique(lens):
        grp = np.nonzero(lens == ln)[0]
        s = int(itab[ln]); g_spr = (int(ln) - L) // s + 1
        for strand in (0, 1):
            ks, rs = _expected(orc, hidx, reads[grp, :ln], int(ln), L, s, strand)
            want_keys[strand].append((grp[ks >> 34].astype(np.int64) << 34) | (ks & ((1 << 34) - 1)))
            for sid, xy in rs.items():
                want_res[strand][int(grp[sid // g_spr]) * spr + sid % g_spr] = xy
    on, off = _run(amd, fmi, qs, M, grid_blocks=64), _run(amd, fmi, qs, M, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
    for got, tag in ((on, "on"), (off, "off")):
        for strand in (0, 1):
            keys = got["keys"]
            assert np.array_equal(np.sort(keys[((keys >> 33) & 1) == strand]), np.sort(np.concatenate(want_keys[strand]))), (k, tag, strand)
        assert got["res"] == want_res, (k, tag)
    _same(on, off, k)
    deferred = 0
    for h, defer in ((1, False), (4, False), (1, True), (4, True)):
        a = _run(amd, fmi, qs, M, inline_hits=h, defer=defer, grid_blocks=64)
        b = _run(amd, fmi, qs, M, inline_hits=h, defer=defer, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
        _same(a, b, (k, h, defer))
        if defer:
            deferred += len(a["keys"]) - a["in_tiles"]
    cnt = _run(amd, fmi, qs, M, grid_blocks=64, flags=amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS)
    _same(cnt, off, (k, "count"))
    placed, settled, gathered, unplaced = cnt["routes"]
    through_group = _anchors_through_a_group(big["text"], reads, L, k, k == 15)      # (every read keeps its first seed: 100 symbols or more)
    print("k", k, "ragged reads", R, "routes", cnt["routes"], "anchors through a group", through_group, "deferred keys", deferred)
    assert placed > 0 and settled > 0 and gathered > 0 and unplaced > 0 and through_group > 0 and deferred > 0


# 256 s + d tiles for s = 0 .. STAGES + 1 and d in {0, 1, 255}: every wave owns s tiles, the first d of them one more -- fewer tiles than
# stages, as many, more.  (0 tiles is a batch without reads: the call launches nothing.)
FILL_DRAIN = [WAVES * s + d for s in range(STAGES + 2) for d in (0, 1, 255) if WAVES * s + d > 0]


@pytest.mark.parametrize("tiles", FILL_DRAIN)
def test_fill_and_drain(amd, orc, big, tiles):
    """a partial last tile; the path on and off against the operators, with DEFER on and off"""
    k = 15
    L, fmi, pool = _seed_len(k), big["fmi"][k], big["pool"][k]
    spr = (M - L) // S + 1
    rpt = 64 // spr
    R = tiles * rpt - 3
    assert R <= len(pool["reads"])
    qs = _uniform_set(amd, orc, pool["reads"][:R], L)
    want, res = _prefix_expected(pool, R, spr)
    on, off = _run(amd, fmi, qs, M, grid_blocks=64), _run(amd, fmi, qs, M, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
    for got, tag in ((on, "on"), (off, "off")):
        assert np.array_equal(got["keys"], want), (tiles, tag)
        assert got["res"] == res, (tiles, tag)
    _same(on, off, tiles)
    assert len(on["tile_offsets"]) == tiles + 1
    a = _run(amd, fmi, qs, M, inline_hits=4, defer=True, grid_blocks=64)
    b = _run(amd, fmi, qs, M, inline_hits=4, defer=True, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
    _same(a, b, (tiles, "defer"))


@pytest.mark.parametrize("defer", [False, True])
def test_the_output_does_not_depend_on_the_grid(amd, orc, big, defer):
    """64 workgroups, 128, and the library's own choice: the same arrays (the deferred searches' keys, appended workgroup by workgroup, as a set)"""
    k = 15
    L, fmi, pool = _seed_len(k), big["fmi"][k], big["pool"][k]
    qs = _uniform_set(amd, orc, pool["reads"], L)
    runs = [_run(amd, fmi, qs, M, inline_hits=4, defer=defer, grid_blocks=gb) for gb in (64, 128, 0)]
    for other in runs[1:]:
        _same(runs[0], other, defer)
        if not defer:
            assert np.array_equal(runs[0]["keys"], other["keys"])


# read length - seed length, seed interval -> 1, 2, 9 and 64 seeds per read: tiles of 64, 32, 7 and 1 reads
SEEDS_PER_READ = {1: (0, 1), 2: (18, 18), 9: (128, 16), 64: (63, 1)}


@pytest.mark.parametrize("k", [9, 15])
@pytest.mark.parametrize("spr", list(SEEDS_PER_READ))
def test_seeds_per_read_in_the_steady_state(amd, orc, big, spr, k):
    """the lane <-> read map decides which lane is an anchor and whom it tells: nine tiles per wave for each"""
    rng = np.random.default_rng(1530 + 7 * spr + k)
    L, fmi, text = _seed_len(k), big["fmi"][k], big["text"]
    extra, s = SEEDS_PER_READ[spr]
    m = L + extra
    assert (m - L) // s + 1 == spr
    R = 9 * WAVES * (64 // spr) - 1
    starts = rng.integers(0, N_BIG - m, R)
    starts[:R // 8] = 30000 + 1000 * rng.integers(0, 12, R // 8) + rng.integers(-60, 280, R // 8)       # the 12-copy family: heavy k-mers
    starts[R // 8:R // 4] = 50000 + 700 * rng.integers(0, 3, R // 4 - R // 8) + rng.integers(-60, 180, R // 4 - R // 8)   # the 3-copy family: groups
    reads = _mix_strands(rng, _take(text, starts, m))
    mut = rng.random(reads.shape) < 0.01
    reads[mut] = (reads[mut] + 1) % 4
    qs = _uniform_set(amd, orc, reads, L, m, s)
    want_f, res_f = _expected(orc, big["hidx"], reads, m, L, s, 0)
    want_r, res_r = _expected(orc, big["hidx"], reads, m, L, s, 1)
    want = _tile_major(want_f, want_r, 64 // spr)
    on, off = _run(amd, fmi, qs, m, grid_blocks=64), _run(amd, fmi, qs, m, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
    for got, tag in ((on, "on"), (off, "off")):
        assert np.array_equal(got["keys"], want), (spr, k, tag)
        assert got["res"] == [res_f, res_r], (spr, k, tag)
    _same(on, off, (spr, k))
    a = _run(amd, fmi, qs, m, inline_hits=4, defer=True, grid_blocks=64)
    b = _run(amd, fmi, qs, m, inline_hits=4, defer=True, grid_blocks=64, flags=amd.FM_NO_SEED_LOCUS)
    _same(a, b, (spr, k, "defer"))
    if spr > 1:
        cnt = _run(amd, fmi, qs, m, grid_blocks=64, flags=amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS)
        assert cnt["routes"][1] > 0, cnt["routes"]
