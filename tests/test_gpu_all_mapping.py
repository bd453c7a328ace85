"""GPU parity of nvBowtie's all-mapping mode: the kernels one by one (scan, select, output) against numpy, and the host loop
(nvbio_host_all_mapping behind amd.all_mapping) against the oracle's read-by-read, pass-by-pass restatement (tests/all_mapping_cpu.py).
All comparisons are exact."""
import math

import numpy as np
import pytest

import oracle
from all_mapping_cpu import all_mapping_cpu, band_length, shared_input

pytestmark = pytest.mark.gpu

EXPAND_TILE = 2048


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


# ---- 1. kernels one by one --------------------------------------------------------------------------------------------------
def _hand_made_ranges(rng, R, spr):
    def ranges():
        x = rng.integers(0, 3_000_000_000, (R, spr))
        size = rng.choice([0, 0, 0, 1, 1, 2, 3, 40], (R, spr))
        return x, size
    (fx, fs), (rx, rs) = ranges(), ranges()
    fs[3, 1] = 5000                                                  # several tiles of EXPAND_TILE
    fs[5], rs[5] = 0, 0                                              # a read whose seeds are all empty
    fs[0, 0], rs[0, 0] = 0, 0
    rs[R - 1, spr - 1] = 7                                           # the last slot is not empty
    pack = lambda x, s: np.stack([np.where(s == 0, 1, x), np.where(s == 0, 0, x + s - 1)], axis=2).astype(np.uint32)
    return pack(fx, fs), pack(rx, rs)


def _expected_hits(fw, rc, R, spr, first, S, L, M):
    """numpy: the scan and every hit (read, SA row, packed_seed) in hit order"""
    j = np.arange(spr)
    in_read = first + j * S + L <= M
    size = lambda g: np.where((g[:, :, 0] <= g[:, :, 1]) & in_read[None, :], (g[:, :, 1].astype(np.int64) + 1 - g[:, :, 0]) & 0xFFFFF, 0)
    sizes = np.stack([size(fw), size(rc)], axis=2).reshape(-1)       # read-major, seed, forward before reverse-complement
    slots = np.cumsum(sizes).astype(np.uint64)
    o = np.arange(int(slots[-1]), dtype=np.uint64)
    i = np.searchsorted(slots, o, side="right")
    base = np.where(i > 0, slots[np.maximum(i, 1) - 1], 0).astype(np.uint64)
    e, strand = i >> 1, i & 1
    read, jj = e // spr, e % spr
    x = np.where(strand == 1, rc.reshape(-1, 2)[e, 0], fw.reshape(-1, 2)[e, 0]).astype(np.uint64)
    off = first + jj * S
    pos = np.where(strand == 1, off, M - off - L)
    return slots, read.astype(np.uint32), ((x + o - base) & 0xFFFFFFFF).astype(np.uint32), (pos | (strand << 13)).astype(np.uint32)


@pytest.mark.parametrize("spr,first", [(6, 8), (8, 8)])              # (8, 8): the last two seed slots end past the read
def test_scan_and_select_equal_numpy(amd, spr, first):
    import torch
    rng = np.random.default_rng(5)
    R, S, L, M = 300, 12, 22, 100
    fw, rc = _hand_made_ranges(rng, R, spr)
    slots_w, read_w, row_w, seed_w = _expected_hits(fw, rc, R, spr, first, S, L, M)
    n_hits = int(slots_w[-1])
    assert n_hits > 3 * EXPAND_TILE
    p = amd.AllHitsParams(spr, first, S, L, M)
    fw_d, rc_d = _dev(fw), _dev(rc)
    slots, n_dev = amd.all_hits_scan(fw_d, rc_d, R, p)
    assert int(n_dev.item()) == n_hits
    assert np.array_equal(slots.cpu().numpy().view(np.uint64), slots_w)
    cut = int(slots_w[2 * (3 * spr + 1)]) - 1234                     # inside the range of 5,000 rows
    batch = 3000
    chunks = [(0, n_hits), (cut, cut + 700), (0, cut), (cut, n_hits)] + [(b, min(b + batch, n_hits)) for b in range(0, n_hits, batch)]
    assert (n_hits % batch) != 0                                     # the last chunk is shorter than the batch
    for begin, end in chunks:
        room = max(batch, end - begin)
        hits = amd.HitQueues(*[torch.full((room,), -1, dtype=torch.int32, device="cuda:0") for _ in range(3)])
        amd.all_hits_select(fw_d, rc_d, R, p, slots, begin, end, hits)
        k = end - begin
        assert np.array_equal(amd.u32(hits.read_id)[:k], read_w[begin:end]), (begin, end)
        assert np.array_equal(amd.u32(hits.loc)[:k], row_w[begin:end]), (begin, end)
        assert np.array_equal(amd.u32(hits.seed)[:k], seed_w[begin:end]), (begin, end)
        assert (amd.u32(hits.read_id)[k:] == 0xFFFFFFFF).all()       # nothing written past the chunk


def test_scan_of_empty_ranges(amd):
    R, spr = 40, 6
    empty = np.tile(np.array([1, 0], dtype=np.uint32), (R, spr, 1))
    slots, n = amd.all_hits_scan(_dev(empty), _dev(empty), R, amd.AllHitsParams(spr, 8, 12, 22, 100))
    assert int(n.item()) == 0 and not slots.cpu().numpy().any()


def test_output_appends_in_hit_order(amd):
    import torch
    rng = np.random.default_rng(9)
    n1, n2, cap, min_score = 5000, 3001, 3000, -3
    out = (torch.full((cap,), -1, dtype=torch.int32, device="cuda:0"), torch.full((cap,), 255, dtype=torch.uint8, device="cuda:0"),
           torch.full((cap,), -1, dtype=torch.int32, device="cuda:0"), torch.full((cap,), 99, dtype=torch.int32, device="cuda:0"))
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    want, total = [], 0
    for n in (n1, n2):                                               # the second call appends at a non-zero offset and overflows the capacity
        rid = rng.integers(0, 1000, n).astype(np.uint32); rcs = rng.integers(0, 2, n).astype(np.uint32)
        loc = rng.integers(0, 4_000_000_000, n).astype(np.uint32); sc = rng.integers(-8, 1, n).astype(np.int32)
        hits = amd.HitQueues(_dev(rid), _dev(((rcs << 13) | 17).astype(np.uint32)), _dev(loc))
        amd.all_score_output(hits, _dev(sc), min_score, out, total, count)
        keep = sc >= min_score
        want.append(np.stack([rid[keep], rcs[keep], loc[keep], sc[keep].astype(np.int64) & 0xFFFFFFFF], axis=1))
        total += int(keep.sum())
        assert int(count.item()) == total                            # the count is kept past the capacity
    want = np.concatenate(want)
    assert total == len(want) > cap
    got = np.stack([amd.u32(out[0]), out[1].cpu().numpy(), amd.u32(out[2]), amd.u32(out[3])], axis=1).astype(np.int64)
    assert np.array_equal(got, want[:cap].astype(np.int64))          # hit order; the records past the capacity are dropped


# ---- 2-6. the loop against the restatement ------------------------------------------------------------------------------------------
class _World:
    def __init__(self, amd, orc):
        import torch
        self.text, self.reads, _ = shared_input()
        self.G = len(self.text)
        self.R, self.M = self.reads.shape
        self.hidx = orc.build_index(self.text)
        genome2 = orc.pack2(self.text)
        self.fmi = amd.FMIndex.build(genome2, self.G, kmer_len=8, sa_int=4)
        self.genome = torch.from_numpy(genome2.view(np.int32)).cuda()
        stored = np.ascontiguousarray(self.reads[:, ::-1])
        self.reads4 = torch.from_numpy(orc.pack4(stored.reshape(-1)).view(np.int32)).cuda()
        self._want = {}
        self.orc = orc

    def want(self, aln_type, max_dist, cigars=False):
        key = (aln_type, max_dist)
        if key not in self._want or (cigars and self._want[key][1] is None):
            if cigars:
                self._want[key] = all_mapping_cpu(self.orc, self.hidx, self.text, self.G, self.reads, aln_type, max_dist, want_cigars=True)
            else:
                self._want[key] = (all_mapping_cpu(self.orc, self.hidx, self.text, self.G, self.reads, aln_type, max_dist), None)
        return self._want[key]

    def run(self, amd, aln_type=oracle.SEMI_GLOBAL, max_dist=15, capacity=20000, **kw):
        cig = kw.pop("want_cigars", False)
        return amd.all_mapping(self.fmi, self.genome, self.G, self.reads4, self.R, self.M, amd.AllMappingParams(aln_type=aln_type, max_dist=max_dist, **kw),
                               capacity, want_cigars=cig)


@pytest.fixture(scope="module")
def world(amd, orc):
    w = _World(amd, orc)
    yield w
    w.fmi.close()


def _records(res):
    return np.stack([res["read_id"].cpu().numpy().view(np.uint32), res["rc"].cpu().numpy(), res["loc"].cpu().numpy().view(np.uint32),
                     res["score"].cpu().numpy()], axis=1).astype(np.int64)


def _sorted(a):
    a = np.asarray(a, dtype=np.int64).reshape(-1, 4)
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("aln_type", [oracle.SEMI_GLOBAL, oracle.LOCAL])
@pytest.mark.parametrize("max_dist", [15, 3])
def test_loop_equals_the_restatement(amd, world, aln_type, max_dist):
    assert band_length(max_dist) == (31 if max_dist == 15 else 7)
    want, _ = world.want(aln_type, max_dist)
    got = world.run(amd, aln_type, max_dist)
    assert got["n_alignments"] == len(want) and got["n_scored"] == got["n_hits"] >= len(want) and got["chunks"] == 1
    a = _records(got)
    assert np.array_equal(_sorted(a), _sorted(want))
    assert (np.diff(a[:, 0]) >= 0).all()                              # read-major: ascending read ids


@pytest.mark.parametrize("aln_type,max_dist", [(oracle.SEMI_GLOBAL, 15), (oracle.LOCAL, 15), (oracle.SEMI_GLOBAL, 3), (oracle.LOCAL, 3)])
def test_cigars_equal_the_restatement(amd, world, aln_type, max_dist):
    want, det = world.want(aln_type, max_dist, cigars=True)
    got = world.run(amd, aln_type, max_dist, want_cigars=True)
    half = band_length(max_dist) // 2
    assert got["n_alignments"] == len(want)
    a = _records(got)
    src = got["source"].cpu().numpy().view(np.uint32).astype(np.int64); snk = got["sink"].cpu().numpy().view(np.uint32).astype(np.int64)
    ed = got["ed"].cpu().numpy().view(np.uint32); cig = got["cigars"].cpu().numpy().view(np.uint16); lens = got["cigar_lens"].cpu().numpy()
    wb = got["win_begin"].cpu().numpy().view(np.uint32)
    go = sorted(range(len(a)), key=lambda k: (tuple(a[k]), int(src[k, 0])))
    wo = sorted(range(len(want)), key=lambda k: (tuple(want[k]), det[k][0][0]))
    for g, w in zip(go, wo):
        assert tuple(a[g]) == tuple(want[w])
        wsrc, wsnk, wed, wcig = det[w]
        assert tuple(src[g]) == wsrc and tuple(snk[g]) == wsnk and ed[g] == wed, (g, w)
        assert lens[g] == len(wcig) and np.array_equal(cig[g, :lens[g]], wcig), (g, w)
        loc = int(a[g, 2])
        assert wb[g] == (loc - half if loc > half else 0)


def test_chunking_changes_nothing(amd, world):
    one = world.run(amd)
    hb = one["n_hits"] // 7 + 1
    assert one["n_hits"] % hb != 0
    many = world.run(amd, hits_per_batch=hb)
    assert many["chunks"] == 7 and many["n_alignments"] == one["n_alignments"] and many["n_hits"] == one["n_hits"]
    assert np.array_equal(_records(many), _records(one))             # the same records in the same order
    short = world.run(amd, capacity=1000, hits_per_batch=hb)         # capacity overflow: the count is kept, the first records are
    assert short["n_alignments"] == one["n_alignments"] and np.array_equal(_records(short), _records(one)[:1000])


def test_per_seed_passes_give_the_same_multiset(amd, world):
    want, _ = world.want(oracle.SEMI_GLOBAL, 15)
    got = world.run(amd, per_seed_passes=True)
    assert got["chunks"] == 6                                        # seed indices 6 and 7 of 8 have no seed at 100 bp
    assert np.array_equal(_sorted(_records(got)), _sorted(want))


def test_unique_gives_the_distinct_records(amd, world):
    want, _ = world.want(oracle.SEMI_GLOBAL, 15)
    got = world.run(amd, unique=True)
    distinct = _sorted(sorted(set(want)))
    assert np.array_equal(_records(got), distinct)                   # sorted by (read_id, rc, loc) as they come
    assert got["n_scored"] < got["n_hits"] and got["n_alignments"] == len(distinct)


def test_python_wrappers_and_host_loop_agree(amd, world):
    """the loop written out over the five kernel wrappers, in two chunks, against nvbio_host_all_mapping"""
    import torch
    R, M, L = world.R, world.M, 22
    S = int(1 + 1.15 * math.sqrt(M)); first = 2 * (S // 3)
    spr = sum(1 for j in range(M // S) if first + j * S + L <= M)
    band, max_dist = 31, 15
    p = amd.AllHitsParams(spr, first, S, L, M)
    offs = (np.arange(R) * M + first).astype(np.uint32)
    qs = amd.PackedStringSet(world.reads4, 4, R * spr, offsets=offs, fixed_len=L, stride=M, seeds_per_string=spr, seed_interval=S)
    fw = world.fmi.match(qs, amd.FM_SCAN_FORWARD); rc = world.fmi.match(qs, amd.FM_COMPLEMENT)
    slots, n_dev = amd.all_hits_scan(fw, rc, R, p)
    n_hits = int(n_dev.item())
    cap = 20000
    out = (torch.zeros(cap, dtype=torch.int32, device="cuda:0"), torch.zeros(cap, dtype=torch.uint8, device="cuda:0"),
           torch.zeros(cap, dtype=torch.int32, device="cuda:0"), torch.zeros(cap, dtype=torch.int32, device="cuda:0"))
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    read_index = (np.arange(R + 1) * M).astype(np.uint32)
    half = n_hits // 2 + 3
    total = 0
    for begin, end in ((0, half), (half, n_hits)):
        n = end - begin
        hits = amd.HitQueues(torch.empty(n, dtype=torch.int32, device="cuda:0"), torch.empty(n, dtype=torch.int32, device="cuda:0"),
                             torch.empty(n, dtype=torch.int32, device="cuda:0"))
        amd.all_hits_select(fw, rc, R, p, slots, begin, end, hits)
        amd.seed_hits_loc(world.fmi.locate(hits.loc), hits)
        rid, flags, wb, we = amd.score_stream_flatten(hits, read_index, band, world.G, reads_reversed=True)
        batch = amd.AlignmentBatch(world.reads4, 4, read_index, world.genome, 2, wb, we, read_id=rid, flags=flags, max_read_len=M)
        scores, _ = amd.batch_banded_alignment_score(band, amd.make_edit_distance_aligner(amd.SEMI_GLOBAL), batch)
        amd.all_score_output(hits, scores, -max_dist, out, total, count)
        total = int(count.item())
    host = world.run(amd)
    assert host["n_hits"] == n_hits and host["n_alignments"] == total
    got = np.stack([amd.u32(out[0][:total]), out[1][:total].cpu().numpy(), amd.u32(out[2][:total]), out[3][:total].cpu().numpy()], axis=1).astype(np.int64)
    assert np.array_equal(got, _records(host))
    # the traceback windows of the accepted records are the scoring windows recomputed
    rid, flags, wb, we = amd.all_traceback_flatten(out[0][:total], out[1][:total], out[2][:total], read_index, band, world.G)
    loc = got[:, 2]
    assert np.array_equal(amd.u32(rid), got[:, 0]) and np.array_equal(flags.cpu().numpy(), np.where(got[:, 1] == 1, 2, 1))
    wb_w = np.where(loc > band // 2, loc - band // 2, 0)
    assert np.array_equal(amd.u32(wb), wb_w) and np.array_equal(amd.u32(we), np.minimum(wb_w + band + M, world.G))
