"""GPU: nvbio_finish_reads -- best, second best, unpack and mapping quality of a tile-ordered candidate list in one launch -- against the
composition it replaces (best_candidate_reduce, best_candidate_unpack, second_candidate_reduce, mapq), bit for bit; the device check of its
precondition; and pipeline.seed_and_extend with the switch on and off."""
import ctypes
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RPT = 7                                  # reads per tile
M = 150
OUTS = ("best", "second", "best_score", "best_pos", "best_rc", "mapq", "second_score")


def _tiles_per_group(amd):
    t = ctypes.c_uint32(0)
    assert amd.lib().nvbio_finish_reads_tiles_per_group(ctypes.c_uint32(RPT), ctypes.byref(t)) == 0
    return int(t.value)


def _candidates(rng, n_tiles, R, lo, hi, empty_tile=None):
    """a candidate list in tile order: per tile the forward candidates of its reads, then the reverse ones.  Read r follows pattern r % 8:
    0 none | 1 one forward | 2 two reverse, far apart | 3 two on one strand closer than M / 2 (the second must be rejected) | 4 two closer
    than M / 2 on opposite strands (the second must be kept) | 5 three that tie on the whole key and one distinct | 6 forty (a repeat) |
    7 one to five at random, some below the threshold.  -> (rid, strand, score, wb, sink_x) per candidate, tile_offsets"""
    per_tile = [[] for _ in range(n_tiles)]
    for r in range(R):
        t = r // RPT
        if t == empty_tile:
            continue
        base = int(rng.integers(2000, 1 << 30))
        sc = lambda: int(rng.integers(lo, hi + 1))
        pat = r % 8
        c = []
        if pat == 1:
            c = [(0, sc(), base, 160)]
        elif pat == 2:
            c = [(1, sc(), base, 160), (1, sc(), base + 5000, 158)]
        elif pat == 3:
            c = [(0, hi, base, 160), (0, hi - 1, base + 20, 161)]
        elif pat == 4:
            c = [(1, hi, base, 160), (0, hi - 1, base + 20, 161)]
        elif pat == 5:
            s = sc()
            c = [(1, s, base, 150), (1, s, base - 10, 160), (1, s, base + 5, 145), (0, lo + (hi - lo) // 2, base + 900, 150)]
        elif pat == 6:
            c = [(int(rng.integers(0, 2)), sc(), base + 400 * j, int(rng.integers(140, 181))) for j in range(40)]
        elif pat == 7:
            c = [(int(rng.integers(0, 2)), int(rng.integers(lo - 30, hi + 1)), base + int(rng.integers(0, 300)), int(rng.integers(140, 181)))
                 for _ in range(int(rng.integers(1, 6)))]
        per_tile[t] += [(r,) + x for x in c]
    rows, offs = [], [0]
    for t in range(n_tiles):
        rows += [x for x in per_tile[t] if x[1] == 0] + [x for x in per_tile[t] if x[1] == 1]
        offs.append(len(rows))
    return np.array(rows, dtype=np.int64).reshape(-1, 5), np.array(offs, dtype=np.int32)


def _device_lists(torch, rows, offs):
    rid, strand, score, wb, sx = (rows[:, j] for j in range(5))
    keys = torch.from_numpy((rid << 34) | (strand << 33) | (wb + 1024 + 15)).cuda()
    scores = torch.from_numpy(score.astype(np.int32)).cuda()
    sinks = torch.from_numpy(np.stack([sx, np.full_like(sx, M)], axis=1).astype(np.int32)).cuda().contiguous()
    wbt = torch.from_numpy((wb & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()
    return keys, scores, sinks, wbt, torch.from_numpy(offs).cuda()


def _composition(amd, torch, keys, scores, sinks, wb, R, dist, worst, perfect, min_score, monotone, version, read_offsets, min_scores, match):
    top = torch.zeros(R, dtype=torch.int64, device="cuda")
    second = torch.zeros(R, dtype=torch.int64, device="cuda")
    if keys.numel():
        amd.best_candidate_reduce(keys, scores, sinks, wb, top)
    bs, bp, brc = amd.best_candidate_unpack(top)
    if keys.numel():
        amd.second_candidate_reduce(keys, scores, sinks, wb, top, dist, worst, second, read_offsets=read_offsets, min_scores=min_scores)
    q, ss = amd.mapq(top, second, perfect, min_score, monotone, version, read_offsets=read_offsets, min_scores=min_scores, match=match)
    return dict(best=top, second=second, best_score=bs, best_pos=bp, best_rc=brc, mapq=q, second_score=ss)


# (version, match bonus): end-to-end scores (match 0: the monotone form) and local ones (match 2: the non-monotone form)
MODES = [(2, 0, False), (2, 2, False), (3, 0, False), (3, 2, False), (2, 0, True)]


@pytest.mark.parametrize("version,match,ragged", MODES, ids=["v2-monotone", "v2", "v3-monotone", "v3", "v2-ragged"])
@pytest.mark.parametrize("tiles", ["one", "two", "group+1"])
def test_finish_reads_equals_the_composition(amd, tiles, version, match, ragged):
    import torch
    tpg = _tiles_per_group(amd)
    n_tiles = {"one": 1, "two": 2, "group+1": tpg + 1}[tiles]
    R = n_tiles * RPT - (0 if tiles == "one" else 3)                          # the last tile partial
    rng = np.random.default_rng(7000 + n_tiles * 10 + version + match)
    if match == 0:
        perfect, min_score = 0, int(np.float32(-0.6) + np.float32(-0.6) * np.float32(M))
    else:
        perfect, min_score = match * M, int(np.float32(10.0) * np.float32(np.log(np.float32(M))))
    rows, offs = _candidates(rng, n_tiles, R, min_score, perfect, empty_tile=1 if n_tiles > 2 else None)
    keys, scores, sinks, wb, toffs = _device_lists(torch, rows, offs)
    read_offsets = min_scores = None
    if ragged:
        lens = rng.integers(100, M + 1, R)
        read_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).cuda()
        min_scores = torch.from_numpy((np.float32(-0.6) + np.float32(-0.6) * lens.astype(np.float32)).astype(np.int32)).cuda()
    want = _composition(amd, torch, keys, scores, sinks, wb, R, M // 2, min_score - 1, perfect, min_score, match == 0, version,
                        read_offsets, min_scores, match)
    got = amd.finish_reads(keys, scores, sinks, wb, toffs, RPT, R, M // 2, min_score - 1, perfect, min_score, match == 0, version,
                           read_offsets=read_offsets, min_scores=min_scores, match=match)
    for k in OUTS:
        assert torch.equal(got[k], want[k]), k
    # the cases the list was built for did occur: a rejected and a kept second, reads without candidates, a span of more than 256 candidates
    sec = got["second"].cpu().numpy()
    r = np.arange(R)
    live = (r // RPT != 1) if n_tiles > 2 else np.ones(R, dtype=bool)
    if not ragged:
        assert (sec[(r % 8 == 3) & live] == 0).all() and (sec[(r % 8 == 4) & live] != 0).all()
    assert (got["best"].cpu().numpy()[r % 8 == 0] == 0).all() and (got["best_pos"].cpu().numpy()[r % 8 == 0] == -1).all()
    if tiles == "group+1":
        assert offs[tpg] - offs[0] > 512                                     # more candidates than the kernel keeps in registers


def test_finish_reads_one_candidate_and_none(amd):
    import torch
    R = 5
    toffs1 = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    rows = np.array([[3, 1, -12, 5000, 160]], dtype=np.int64)
    keys, scores, sinks, wb, _ = _device_lists(torch, rows, np.array([0, 1], dtype=np.int32))
    for k, s, x, w, t in ((keys, scores, sinks, wb, toffs1),
                          (keys[:0], scores[:0], sinks[:0], wb[:0], torch.zeros(2, dtype=torch.int32, device="cuda"))):
        want = _composition(amd, torch, k, s, x, w, R, 75, -91, 0, -90, True, 2, None, None, 0)
        got = amd.finish_reads(k, s, x, w, t, RPT, R, 75, -91, 0, -90, True, 2)
        for name in OUTS:
            assert torch.equal(got[name], want[name]), name
    assert amd.finish_reads(keys[:0], scores[:0], sinks[:0], wb[:0], toffs1[:1], RPT, 0, 75, -91, 0, -90, True, 2)["best"].numel() == 0


def test_finish_reads_reports_a_list_out_of_tile_order(amd):
    """one candidate of the last tile moved into the first tile's span (another workgroup's): the device flags it and the wrapper raises;
    so it does for a list longer than the spans (keys appended behind the tiles).  An ordinary flagged return: nothing faults."""
    import torch
    tpg = _tiles_per_group(amd)
    n_tiles = tpg + 1
    R = n_tiles * RPT
    rng = np.random.default_rng(77)
    rows, offs = _candidates(rng, n_tiles, R, -90, 0)
    args = (RPT, R, M // 2, -91, 0, -90, True, 2)
    moved = np.concatenate([rows[-1:], rows[:-1]])
    moffs = offs.copy(); moffs[1:-1] += 1
    with pytest.raises(RuntimeError, match="tile order"):
        amd.finish_reads(*_device_lists(torch, moved, moffs), *args)
    keys, scores, sinks, wb, toffs = _device_lists(torch, rows, offs)
    short = toffs.clone(); short[-1] -= 1                                      # the last candidate behind every span
    with pytest.raises(RuntimeError, match="tile order"):
        amd.finish_reads(keys, scores, sinks, wb, short, *args)
    amd.finish_reads(keys, scores, sinks, wb, toffs, *args)                   # the flag does not stick to a later, well-formed call


def _mapping_case(amd, orc, rng, repeat):
    import torch
    pipeline = importlib.import_module("nvbio_gpl_amd.pipeline")
    G, R = 200_000, 5000
    text = rng.integers(0, 4, G, dtype=np.uint8)
    if repeat:
        unit = rng.integers(0, 4, 300, dtype=np.uint8)
        for c in range(12):
            text[30000 + 5000 * c:30300 + 5000 * c] = unit
    starts = rng.integers(0, G - M - 8, R)
    if repeat:
        starts[:400] = 30000 + 5000 * rng.integers(0, 12, 400) + rng.integers(0, 150, 400)
    reads = np.empty((R, M), dtype=np.uint8)
    for i, s in enumerate(starts):
        w = text[s:s + M + 8].copy()
        mut = rng.random(M + 8) < 0.01
        w[mut] = (w[mut] + 1 + rng.integers(0, 3, int(mut.sum()))) % 4
        if i % 5 == 0:                                                         # a deletion or an insertion in the read
            p = int(rng.integers(30, 120))
            w = np.delete(w, p) if i % 10 == 0 else np.insert(w, p, rng.integers(0, 4))
        reads[i] = w[:M]
    rcm = rng.random(R) < 0.5
    reads[rcm] = 3 - reads[rcm][:, ::-1]
    genome2 = orc.pack2(text)
    fmi = amd.FMIndex.build(genome2, G, kmer_len=11, sa_int=1, table_flags=amd.FM_TABLE_CANONICAL_WIDE)
    g_dev = torch.from_numpy(genome2.view(np.int32)).cuda()
    rb = pipeline.ReadBatch(torch.from_numpy(orc.pack4(reads.reshape(-1)).view(np.int32)).cuda(), R, M)
    runs = []
    for fused in (True, False):
        params = pipeline.SeedExtendParams.end_to_end(seed_len=16)
        params.mapq, params.fused_finish = True, fused
        timers, extras = {}, {}
        out = pipeline.seed_and_extend(fmi, g_dev, G, rb, params, timers, return_windows=True, extras=extras)
        amd.FinishStatus.of(g_dev.device).check(wait=True)
        runs.append((out, extras, set(timers)))
    fmi.close()
    return runs


@pytest.mark.parametrize("repeat", [False, True], ids=["unique", "planted-repeat"])
def test_seed_and_extend_with_and_without_the_fused_finish(amd, orc, repeat):
    import torch
    (out_f, ex_f, names_f), (out_o, ex_o, names_o) = _mapping_case(amd, orc, np.random.default_rng(901 + repeat), repeat)
    assert {"reduce", "unpack", "mapq"} <= names_o and "finish" not in names_o
    if repeat:                                                                # residual keys: not in tile order, the separate kernels run
        assert "locate" in names_f and {"reduce", "unpack", "mapq"} <= names_f and "finish" not in names_f
    else:
        assert "finish" in names_f and not ({"reduce", "unpack", "mapq"} & names_f)
    assert out_f[3] == out_o[3] and out_f[3] > 0
    for a, b in zip(out_f[:3] + out_f[4:], out_o[:3] + out_o[4:]):
        assert torch.equal(a, b)
    assert set(ex_f) == set(ex_o) and {"mapq", "second_score", "second", "best_keys"} <= set(ex_f)
    for k in ex_f:
        assert torch.equal(ex_f[k], ex_o[k]), k
    assert int((ex_f["second"] != 0).sum()) > 0 or not repeat
