"""The two ways a tile of the two-strand seed pass is resolved (csrc/fm_canon_inl.h: resolve_tile): the common path -- rows by counts, one
emission for both strands -- and the general code.  Every batch runs by default, with FM_NO_FAST_RESOLVE (the general code everywhere) and
against the per-strand operators of the oracle; keys in order, tile spans, residual lists, the deferred searches' keys and the counts must
agree, with the locus path on and off, DEFER on and off, in-line hits 1 and 4, and both table widths.

Which path a tile takes is predicted on the CPU from the text alone: a lane is uncommon iff its seed is clean and either the k-mer the
table is asked for (the seed's last k symbols) has more than 8 occurrences over both strands, or the seed has more than one hit over both
strands; a tile is common iff it has no such lane.  FM_COUNT_RESOLVE reports the tiles per path (counts[10:12]) of the launch it accounts
for, and every test asserts that these equal the prediction where that launch holds the common path (16-byte entries with DEFER: see
_three_ways) and that every tile took the general code elsewhere: the batches are built so that both paths run, and the counts prove
that they did.

Shapes as in test_gpu_seed_locus_schedule.py: k = 9, seeds of 14 symbols, a text of 40 k symbols, grid_blocks = 64."""
import numpy as np
import pytest

from test_gpu_seed_pass import _expected, _tile_major
from test_seed_locus_layout import occurrences, window_codes

pytestmark = pytest.mark.gpu

K, L = 9, 14
N = 40009
M, S = 150, 16                              # 9 seeds per read: tiles of 7 reads, lanes 0 .. 62
SPR, RPT = 9, 7
FREE = (2200, 19000)                        # text without planted copies
KINDS = ("two_copies", "six_copies", "heavy", "self_complementary")
GROUP_ROWS = (3, 4, 5, 8)


def _rc(a):
    a = np.asarray(a)
    return np.where(a[..., ::-1] < 4, 3 - a[..., ::-1], 4).astype(np.uint8)


def _code(a):
    return sum(a[..., i].astype(np.int64) << (2 * i) for i in range(a.shape[-1]))


class Occurrences:
    """occurrences of a window over the text, per strand"""
    def __init__(self, text, length):
        self.vals, self.cnt = np.unique(window_codes(text, length)[0], return_counts=True)

    def count(self, windows):
        c = _code(windows)
        i = np.minimum(np.searchsorted(self.vals, c), len(self.vals) - 1)
        return np.where(self.vals[i] == c, self.cnt[i], 0)


def _world_text(rng):
    """a random text with: a two-copy element, a six-copy one (more hits than in-line slots, its k-mers not heavy), a 12-copy one (heavy
    k-mers), a window that is its own reverse complement, an element with one reverse-complement copy and one with two, and for
    m = 3, 4, 5, 8 a k-mer with exactly m occurrences whose left flanks are distinct except for one pair"""
    text = rng.integers(0, 4, N, dtype=np.uint8)
    text[20000:20100] = text[1000:1100]
    for c in range(5):
        text[21000 + 100 * c:21040 + 100 * c] = text[1200:1240]
    for c in range(11):
        text[22000 + 100 * c:22040 + 100 * c] = text[1400:1440]
    text[23000 + L // 2:23000 + L] = _rc(text[23000:23000 + L // 2])
    text[24000:24200] = _rc(text[1600:1800])
    text[24300:24400] = _rc(text[1900:2000]); text[24500:24600] = _rc(text[1900:2000])
    groups = {}
    at = 26000
    for m in GROUP_ROWS:
        while True:                                                             # a k-mer the text does not hold on either strand
            kmer = rng.integers(0, 4, K, dtype=np.uint8)
            occ = Occurrences(text, K)
            if occ.count(kmer[None])[0] + occ.count(_rc(kmer)[None])[0] == 0:
                break
        flanks = []
        while len(flanks) < m:                                                  # m - 1 distinct flanks and one of them absent from the text
            f = rng.integers(0, 4, L - K, dtype=np.uint8)
            if not any(np.array_equal(f, g) for g in flanks):
                flanks.append(f)
        absent, flanks = flanks[-1], [flanks[0]] + flanks[:-1]                  # the first flank twice
        for f in flanks:
            text[at:at + L - K], text[at + L - K:at + L] = f, kmer
            at += 40
        groups[m] = {2: np.concatenate([flanks[0], kmer]), 1: np.concatenate([flanks[2], kmer]), 0: np.concatenate([absent, kmer])}
    return text, groups


@pytest.fixture(scope="module")
def world(amd, orc):
    rng = np.random.default_rng(1616)
    text, groups = _world_text(rng)
    w = dict(text=text, groups=groups, hidx=orc.build_index(text), fmi={}, occ_l=Occurrences(text, L), occ_k=Occurrences(text, K))
    for wide in (False, True):
        fmi = amd.FMIndex.build(orc.pack2(text), N, kmer_len=K, sa_int=1, table_flags=amd.FM_TABLE_CANONICAL_WIDE if wide else amd.FM_TABLE_CANONICAL)
        fmi.build_seed_locus(L)
        assert fmi.seed_locus()[1] == L
        w["fmi"][wide] = fmi
    w["repeat_cs"] = np.concatenate([[0], np.cumsum(occurrences(text, L) != 1)])
    w["special"] = dict(two_copies=text[1010:1010 + L].copy(), six_copies=text[1210:1210 + L].copy(), heavy=text[1410:1410 + L].copy(),
                        self_complementary=text[23000:23000 + L].copy())
    yield w
    for fmi in w["fmi"].values():
        fmi.close()


def _lanes(world, seeds, has):
    """per seed window [n, L]: hits on the forward strand, on the reverse strand, occurrences of the k-mer asked for, uncommon or not"""
    clean = has & (seeds < 4).all(axis=1)
    s = np.where(clean[:, None], seeds, 0).astype(np.uint8)
    nf, nr = world["occ_l"].count(s), world["occ_l"].count(_rc(s))
    kocc = world["occ_k"].count(s[:, L - K:]) + world["occ_k"].count(_rc(s[:, L - K:]))
    return nf, nr, kocc, clean & ((kocc > 8) | (nf + nr > 1))


def _predict(world, windows, has, spr):
    """windows [R, spr, L], has [R, spr] -> (lanes' figures reshaped [R, spr], number of tiles, the tiles that take the general code)"""
    R = windows.shape[0]
    nf, nr, kocc, unc = (v.reshape(R, spr) for v in _lanes(world, windows.reshape(-1, L), has.reshape(-1)))
    rpt = 64 // spr
    n_tiles = -(-R // rpt)
    general = np.unique(np.nonzero(unc.any(axis=1))[0] // rpt)
    return (nf, nr, kocc, unc), n_tiles, general


def _run(amd, fmi, qs, m, flags=0, inline_hits=0, defer=False):
    b = fmi.match_seed_diagonals_both(qs, m, flags=flags, inline_hits=inline_hits, defer_heavy=defer, grid_blocks=64)
    c = [int(v) for v in b["counts"][:4].cpu().numpy()]
    res = []
    for lo, cnt in ((0, c[1]), (qs.n, c[2])):
        rr = amd.u32(b["ranges"][lo:lo + cnt]); ids = b["ids"][lo:lo + cnt].cpu().numpy()
        res.append({int(i): (int(a), int(d)) for i, (a, d) in zip(ids, rr)})
    out = dict(keys=b["keys"][:c[0]].cpu().numpy(), counts=c, in_tiles=c[3], res=res, tile_offsets=b["tile_offsets"].cpu().numpy().copy())
    if flags & amd.FM_COUNT_SECTORS:
        out["sectors"] = int(b["counts"][4:6].cpu().numpy().view(np.uint64)[0])
        out["paths"] = [int(v) for v in b["counts"][10:12].cpu().numpy()]
    return out


def _same(a, b, what):
    """two runs left the same: counts, the tiles' keys key for key, the tile spans (the tile counts), the residual lists, and behind the
    tiles the deferred searches' keys (appended workgroup by workgroup: as a set).  The deferred slots and their per-tile counts live in the
    call's scratch and are not handed out; they are held through what they produce: a tile whose deferred count or slots were wrong would
    run other searches, and counts[0] (all keys) or the set of keys behind the tiles would differ."""
    assert a["counts"] == b["counts"], what
    assert np.array_equal(a["keys"][:a["in_tiles"]], b["keys"][:b["in_tiles"]]), what
    assert np.array_equal(np.sort(a["keys"][a["in_tiles"]:]), np.sort(b["keys"][b["in_tiles"]:])), what
    assert np.array_equal(a["tile_offsets"], b["tile_offsets"]), what
    assert a["res"] == b["res"], what


def _three_ways(amd, world, qs, m, n_tiles, general, want, what):
    """default | FM_NO_FAST_RESOLVE | the operators (want: (keys in tile order or per-strand sorted keys, residual lists)), crossed with
    the table width, the locus path, DEFER and the in-line hits; the tiles per path against the prediction.

    Which kernels hold the common path at all (FAST_FORM in fm_canon_inl.h): 4-bit reads over 16-byte entries with DEFER, with the locus
    path or without.  So here the common path runs in the runs with wide = True and defer = True, and in the accounting runs of those
    flags; in every other run default and FM_NO_FAST_RESOLVE are the same general code, and the comparison with the operators at in-line
    hits 1 without DEFER checks that code.  The common path itself is held against the operators tile by tile: a common tile has no
    deferred search, so in a DEFER run its keys are exactly the operators' keys of its reads, in their order."""
    COUNT = amd.FM_COUNT_SECTORS | amd.FM_COUNT_LOCUS | amd.FM_COUNT_RESOLVE
    rpt = 64 // qs.seeds_per_string
    keys, res = want
    ragged = isinstance(keys, list)                                             # ragged reads: per strand, as a set
    want_all = np.concatenate(keys) if ragged else keys
    common = np.setdiff1d(np.arange(n_tiles), general)
    for wide, fmi in world["fmi"].items():
        for locus in (0, amd.FM_NO_SEED_LOCUS):
            tag = (what, "wide" if wide else "narrow", "locus off" if locus else "locus on")
            for h, defer in ((1, False), (4, False), (1, True), (4, True)):
                a = _run(amd, fmi, qs, m, flags=locus, inline_hits=h, defer=defer)
                b = _run(amd, fmi, qs, m, flags=locus | amd.FM_NO_FAST_RESOLVE, inline_hits=h, defer=defer)
                _same(a, b, tag + (h, defer))
                if h == 1 and not defer:
                    if ragged:
                        for strand in (0, 1):
                            assert np.array_equal(np.sort(a["keys"][((a["keys"] >> 33) & 1) == strand]), keys[strand]), tag + (strand,)
                    else:
                        assert np.array_equal(a["keys"], keys), tag
                    assert a["res"] == res, tag
                    plain = a
                if defer:
                    off = a["tile_offsets"]
                    tile_of = (want_all >> 34) // rpt
                    for t in common:
                        got, exp = a["keys"][off[t]:off[t + 1]], want_all[tile_of == t]
                        assert np.array_equal(np.sort(got), np.sort(exp)) if ragged else np.array_equal(got, exp), tag + (h, "tile", t)
            for defer in (False, True):
                fast = _run(amd, fmi, qs, m, flags=locus | COUNT, defer=defer)
                slow = _run(amd, fmi, qs, m, flags=locus | COUNT | amd.FM_NO_FAST_RESOLVE, defer=defer)
                _same(fast, plain, tag + ("count", defer)); _same(slow, plain, tag + ("count, general", defer))
                assert fast["sectors"] == slow["sectors"], tag
                # an accounting run follows the launch it accounts for: the common path only where that launch holds it
                held = wide and defer
                assert fast["paths"] == ([n_tiles - len(general), len(general)] if held else [0, n_tiles]), (tag, defer, fast["paths"], n_tiles, general)
                assert slow["paths"] == [0, n_tiles], (tag, defer, slow["paths"])


def _windows(reads, m, s):
    spr = (m - L) // s + 1
    return np.stack([reads[:, j * s:j * s + L] for j in range(spr)], axis=1)


def _check_uniform(amd, orc, world, reads, what, m=M, s=S):
    R = reads.shape[0]
    spr = (m - L) // s + 1
    windows = _windows(reads, m, s)
    lanes, n_tiles, general = _predict(world, windows, np.ones((R, spr), dtype=bool), spr)
    qs = amd.PackedStringSet(orc.pack4(reads.reshape(-1)), 4, R * spr, fixed_len=L, stride=m, seeds_per_string=spr, seed_interval=s)
    want_f, res_f = _expected(orc, world["hidx"], reads, m, L, s, 0)
    want_r, res_r = _expected(orc, world["hidx"], reads, m, L, s, 1)
    _three_ways(amd, world, qs, m, n_tiles, general, (_tile_major(want_f, want_r, spr), [res_f, res_r]), what)
    return lanes, n_tiles, general, (want_f, want_r)


def _clean_reads(rng, world, R, m=M, strands=True):
    """reads from text without planted copies, every window of which occurs once over both strands (40 k symbols hold a few chance repeats)"""
    text, cs = world["text"], world["repeat_cs"]
    starts = []
    while len(starts) < R:
        s = int(rng.integers(FREE[0], FREE[1] - m))
        if cs[s + m - L + 1] == cs[s]:
            starts.append(s)
    reads = np.stack([text[s:s + m] for s in starts]).copy()
    if strands:
        rcm = rng.random(R) < 0.5
        reads[rcm] = _rc(reads[rcm])
    return reads


def test_common_tiles_only(amd, orc, world):
    """clean reads of both strands, a partial last tile: every tile takes the common path; a read's nine seeds share a diagonal and leave
    one key (adjacent lanes of one read are dropped), both slot ranges of a tile are populated"""
    rng = np.random.default_rng(1)
    reads = _clean_reads(rng, world, 10 * RPT + 3)
    (nf, nr, kocc, unc), n_tiles, general, (wf, wr) = _check_uniform(amd, orc, world, reads, "common")
    assert n_tiles == 11 and len(general) == 0
    assert (nf + nr == 1).all() and len(wf) + len(wr) == len(reads)
    tiles_f, tiles_r = np.unique((wf >> 34) // RPT), np.unique((wr >> 34) // RPT)
    assert len(np.intersect1d(tiles_f, tiles_r)) >= 8
    assert (kocc >= 3).any() and (kocc == 2).any()                              # lanes through a group, and through the second row of a wide entry


@pytest.mark.parametrize("kind", KINDS)
def test_one_uncommon_lane(amd, orc, world, kind):
    """tiles whose ONE uncommon lane sits at lane 0, 1, 8, 9 or 62 -- the first and last seed of the first and last read of a tile, and the
    first seed of its second read -- with common tiles between them"""
    rng = np.random.default_rng(2 + KINDS.index(kind))
    places = (0, 1, 8, 9, 62)
    reads = _clean_reads(rng, world, 2 * len(places) * RPT + 2)
    for t, lane in enumerate(places):
        r, j = 2 * t * RPT + lane // SPR, lane % SPR
        reads[r, j * S:j * S + L] = world["special"][kind]
    (nf, nr, kocc, unc), n_tiles, general, _ = _check_uniform(amd, orc, world, reads, kind)
    assert list(general) == [2 * t for t in range(len(places))]
    assert int(unc.sum()) == len(places)
    for t, lane in enumerate(places):
        r, j = 2 * t * RPT + lane // SPR, lane % SPR
        assert unc[r, j]
        assert {"two_copies": nf[r, j] == 2 and nr[r, j] == 0, "six_copies": nf[r, j] == 6 and kocc[r, j] <= 8,
                "heavy": kocc[r, j] > 8, "self_complementary": nf[r, j] == 1 and nr[r, j] == 1}[kind]


def test_group_lanes(amd, orc, world):
    """group lanes of 3, 4, 5 and 8 rows whose flanks leave 0, 1 and 2 hits, seen from either strand: with 0 or 1 hit the tile stays common,
    and the decision is taken after the group rows"""
    rng = np.random.default_rng(7)
    combos = [(m, hits, rc) for m in GROUP_ROWS for hits in (0, 1, 2) for rc in (False, True)]
    reads = _clean_reads(rng, world, len(combos) * RPT + 5)
    where = []
    for t, (m, hits, rc) in enumerate(combos):
        lane = int(rng.integers(0, RPT * SPR))
        r, j = t * RPT + lane // SPR, lane % SPR
        seed = world["groups"][m][hits]
        reads[r, j * S:j * S + L] = _rc(seed) if rc else seed
        where.append((r, j))
    (nf, nr, kocc, unc), n_tiles, general, _ = _check_uniform(amd, orc, world, reads, "groups")
    for (m, hits, rc), (r, j) in zip(combos, where):
        assert nf[r, j] + nr[r, j] == hits and (nr[r, j] if rc else nf[r, j]) == hits, (m, hits, rc)
        assert rc or kocc[r, j] == m, (m, hits)                                 # (seen from the other strand the lane asks for another k-mer)
    assert list(general) == [t for t, (m, hits, rc) in enumerate(combos) if hits == 2]


def test_orientations_mixed_in_one_group(amd, orc, world):
    """reads from elements that also occur reverse-complemented (once: a hit on both strands; twice: a group of three rows of both
    orientations, one hit on one strand and two on the other)"""
    rng = np.random.default_rng(8)
    text = world["text"]
    starts = np.concatenate([1600 + rng.integers(-100, 160, 4 * RPT), 1900 + rng.integers(-100, 60, 4 * RPT), 24300 + rng.integers(-100, 200, 2 * RPT + 3)])
    reads = np.stack([text[s:s + M] for s in starts]).copy()
    rcm = rng.random(len(reads)) < 0.5
    reads[rcm] = _rc(reads[rcm])
    reads = reads[rng.permutation(len(reads))]
    (nf, nr, kocc, unc), n_tiles, general, _ = _check_uniform(amd, orc, world, reads, "mixed orientations")
    assert ((nf == 1) & (nr == 1)).any() and ((nf == 1) & (nr == 2)).any() and ((nf == 2) & (nr == 1)).any()
    assert 0 < len(general) <= n_tiles


def test_duplicates_and_their_boundaries(amd, orc, world):
    """adjacent lanes of a read on one diagonal (dropped); the same diagonal in neighbouring reads (kept: another read); an indel read (two
    diagonals); a read whose first key's predecessor lies in the previous read (its first seeds have no hit); seeds with N; reads that hang
    over either end of the text on either strand -- in common tiles and, with one two-copy seed planted, in general ones"""
    rng = np.random.default_rng(9)
    text = world["text"]
    out = []
    for strand in (0, 1):
        base = _clean_reads(rng, world, 1, strands=False)[0]
        twin = base.copy()
        late = base.copy(); late[0:2 * S] = (late[0:2 * S] + 1) % 4              # no hit for its first two seeds
        out += [base, twin, late, base]
        s = int(rng.integers(FREE[0], FREE[1] - M - 8))
        out.append(np.concatenate([text[s:s + 70], text[s + 73:s + M + 3]]))    # a deletion from the read
        out.append(np.concatenate([text[s:s + 90], rng.integers(0, 4, 2, dtype=np.uint8), text[s + 90:s + M - 2]]))
        withn = base.copy(); withn[[3, 40, 41, 100]] = 4
        out.append(withn)
        for h in (1, 17, 100):
            junk = rng.integers(0, 4, h, dtype=np.uint8)
            out.append(np.concatenate([text[N - M + h:], junk])); out.append(np.concatenate([junk, text[:M - h]]))
        if strand:
            out[len(out) // 2:] = [_rc(r) for r in out[len(out) // 2:]]
    reads = np.stack(out + list(_clean_reads(rng, world, 3 * RPT - len(out) % RPT + 2)))
    (nf, nr, kocc, unc), n_tiles, general, (wf, wr) = _check_uniform(amd, orc, world, reads, "duplicates")
    assert len(general) == 0
    per_read = np.bincount(np.concatenate([wf, wr]) >> 34, minlength=len(reads))
    assert per_read[0] == per_read[1] == per_read[2] == per_read[3] == 1 and per_read[4] == 2 and per_read[5] == 2
    assert (wf[wf >> 34 == 0] & ((1 << 34) - 1)) == (wf[wf >> 34 == 1] & ((1 << 34) - 1))
    planted = reads.copy()
    for r in range(0, len(reads), RPT):
        planted[r + 1, 4 * S:4 * S + L] = world["special"]["two_copies"]
    (_, _, _, unc), n_tiles, general, _ = _check_uniform(amd, orc, world, planted, "duplicates, general")
    assert len(general) == n_tiles


SEEDS_PER_READ = {1: (0, 1), 2: (18, 18), 9: (136, 16), 64: (63, 1)}            # read length - seed length, seed interval


@pytest.mark.parametrize("spr", list(SEEDS_PER_READ))
def test_seeds_per_read(amd, orc, world, spr):
    """1, 2, 9 and 64 seeds per read (tiles of 64, 32, 7 and 1 reads), reads from clean text and from every planted element"""
    rng = np.random.default_rng(10 + spr)
    text = world["text"]
    extra, s = SEEDS_PER_READ[spr]
    m = L + extra
    assert (m - L) // s + 1 == spr
    R = 24 * (64 // spr) - 1
    starts = rng.integers(FREE[0], FREE[1] - m, R)
    special = rng.random(R) < (0.02 if spr < 9 else 0.3)
    starts[special] = rng.choice([1000, 1200, 1400, 1600, 1900, 20000, 21100, 22300, 22990, 24000, 24310, 26000, 26200], int(special.sum())) + rng.integers(0, 30, int(special.sum()))
    reads = np.stack([text[a:a + m] for a in starts]).copy()
    rcm = rng.random(R) < 0.5
    reads[rcm] = _rc(reads[rcm])
    _, n_tiles, general, _ = _check_uniform(amd, orc, world, reads, ("spr", spr), m, s)
    assert 0 < len(general) < n_tiles


def test_ragged_reads(amd, orc, world):
    """reads of 100 .. 150 symbols, each with its own seed interval (the RAGGED form of the locus loop, q.intervals in the others): clean
    reads and reads with a planted uncommon seed, against the operators length group by length group"""
    rng = np.random.default_rng(11)
    text = world["text"]
    R = 30 * RPT + 4
    full = _clean_reads(rng, world, R)
    lens = rng.integers(100, M + 1, R)
    itab = np.maximum((np.float32(1.0) + np.float32(1.15) * np.sqrt(np.arange(M + 1, dtype=np.float32))).astype(np.int32), 1)
    ivs = itab[lens]
    nseeds = (lens - L) // ivs + 1
    spr = int(nseeds.max())
    rpt = 64 // spr
    for t, kind in enumerate(KINDS + KINDS):                                    # one uncommon seed in every third tile
        r = 3 * t * rpt + int(rng.integers(0, rpt)); j = int(rng.integers(0, nseeds[r]))
        full[r, j * ivs[r]:j * ivs[r] + L] = world["special"][kind]
    windows = np.zeros((R, spr, L), dtype=np.uint8); has = np.zeros((R, spr), dtype=bool)
    for r in range(R):
        for j in range(nseeds[r]):
            windows[r, j], has[r, j] = full[r, j * ivs[r]:j * ivs[r] + L], True
    _, n_tiles, general = _predict(world, windows, has, spr)
    flat = np.concatenate([full[r, :lens[r]] for r in range(R)])
    offs = np.zeros(R + 1, dtype=np.int64); offs[1:] = np.cumsum(lens)
    qs = amd.PackedStringSet(orc.pack4(flat), 4, R * spr, offsets=offs.astype(np.uint32), fixed_len=L, stride=0, seeds_per_string=spr,
                             seed_intervals=ivs.astype(np.uint32))
    want_keys, want_res = [[], []], [{}, {}]
    for ln in np.unique(lens):
        grp = np.nonzero(lens == ln)[0]
        s = int(itab[ln]); g_spr = (int(ln) - L) // s + 1
        for strand in (0, 1):
            ks, rs = _expected(orc, world["hidx"], full[grp, :ln], int(ln), L, s, strand)
            want_keys[strand].append((grp[ks >> 34].astype(np.int64) << 34) | (ks & ((1 << 34) - 1)))
            for sid, xy in rs.items():
                want_res[strand][int(grp[sid // g_spr]) * spr + sid % g_spr] = xy
    want = [np.sort(np.concatenate(k)) for k in want_keys]
    _three_ways(amd, world, qs, M, n_tiles, general, (want, want_res), "ragged")
    assert 0 < len(general) < n_tiles
