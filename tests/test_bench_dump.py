"""bench.py --dump-outputs without a GPU: dtypes, the 64 MB budget and the seeded row sample of dump_outputs, on a stand-in env
that hands out the output arena the way ParkingBatch.download_outputs does."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
import bench  # noqa: E402


class _Env:
    def __init__(self, n, image):
        self.n, self.device, self.image = n, 'cpu', image

    def download_outputs(self):
        n, r = self.n, np.random.default_rng(5)
        out = {'lidar': r.random((n, 120), np.float32), 'action_mask': r.random((n, 42), np.float32),
               'target': r.random((n, 5), np.float32), 'reward': r.random(n, np.float32), 'reward_info': r.random((n, 5), np.float32),
               'status': r.integers(0, 6, n).astype(np.int32), 'done': r.integers(0, 2, n).astype(np.uint8), 'pose': r.random((n, 3)),
               'rs_word': r.integers(-1, 6, (n, 8)).astype(np.int8), 'rs_lengths': r.random((n, 5), np.float32)}
        if self.image:
            out['img'] = r.integers(0, 256, (n, 3, 64, 64)).astype(np.uint8)
        return out


def _dump(tmp_path, monkeypatch, n, image, seed=42):
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    env = _Env(n, image)
    d = str(tmp_path / f'{n}_{image}_{seed}')
    bench.dump_outputs(env, d, seed)
    return env.download_outputs(), {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}, d


def test_dump_keeps_every_row_within_the_budget(tmp_path, monkeypatch):
    src, got, d = _dump(tmp_path, monkeypatch, 65536, False)
    assert set(got) == set(src)                                     # no sample: no scene_index
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.array_equal(v, src[k].astype(v.dtype)), k
    assert got['status'].dtype == np.float64 and got['rs_word'].dtype == np.float32
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_BYTES


def test_dump_above_the_budget_is_one_seeded_row_sample(tmp_path, monkeypatch):
    src, got, d = _dump(tmp_path, monkeypatch, 65536, True)
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_BYTES
    rows = got.pop('scene_index').astype(np.int64)
    assert len(rows) > 1000 and np.all(np.diff(rows) > 0) and rows[-1] < 65536
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.array_equal(v, src[k][rows].astype(v.dtype)), k
    _, again, _ = _dump(tmp_path, monkeypatch, 65536, True, seed=42)
    assert np.array_equal(again['scene_index'], rows)              # same arguments, same sample
