"""CPU: bench.py --dump-outputs writes every array the step returned, in float64, within its byte bound; a batch that does not fit
is written as the same seeded sample of reads every time."""
import os

import numpy as np
import torch

import bench


def _columns(R, seed):
    g = torch.Generator().manual_seed(seed)
    return [("best_score", torch.randint(-300, 1, (R,), generator=g, dtype=torch.int32)),
            ("best_pos", torch.randint(-1, 3_000_000_000, (R,), generator=g, dtype=torch.int64)),
            ("best_rc", torch.randint(0, 2, (R,), generator=g, dtype=torch.uint8)),
            ("tb_cigar", torch.randint(0, 1 << 12, (R, 4), generator=g, dtype=torch.int16))]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_whole_batch_when_it_fits(tmp_path):
    R = 1000
    cols = _columns(R, 1)
    bench.dump_outputs(torch, np, str(tmp_path), R, cols, {"n_candidates": 1234})
    out = _load(str(tmp_path))
    assert sorted(out) == ["best_pos", "best_rc", "best_score", "n_candidates", "read_index", "tb_cigar"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["read_index"], np.arange(R))
    for name, t in cols:
        assert np.array_equal(out[name], t.numpy().astype(np.float64)), name
    assert out["n_candidates"].tolist() == [1234.0]


def test_seeded_sample_within_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1_000_000)
    R = 200_000
    cols = _columns(R, 2)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(torch, np, a, R, cols, {"n_candidates": 7})
    bench.dump_outputs(torch, np, b, R, _columns(R, 2), {"n_candidates": 7})
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 1_000_000
    A, B = _load(a), _load(b)
    idx = A["read_index"].astype(np.int64)
    assert 0 < len(idx) < R and np.all(np.diff(idx) > 0) and idx[-1] < R
    assert all(np.array_equal(A[k], B[k]) for k in A)                       # same arguments, same sample, same arrays
    for name, t in cols:
        assert np.array_equal(A[name], t.numpy()[idx].astype(np.float64)), name
