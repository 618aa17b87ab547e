"""bench.py --dump-outputs (dump_outputs) on CPU tensors: what it writes, that a fixed seed gives the same sample every time,
that the N > 1 gather assembles the same files as one process holding every band, and that the files stay within 64 MB."""
import os

import numpy as np
import torch

import bench


def _maps(k, n_band, bands, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, (n_band,), dtype=torch.int32, generator=g) for _ in range(bands)]


def _load(path):
    return {n[:-4]: np.load(os.path.join(path, n)) for n in sorted(os.listdir(path))}


def test_small_image_is_dumped_whole(tmp_path):
    k, n_band = 16, 1000
    maps = _maps(k, n_band, 2)
    cent = np.arange(k * 4, dtype=np.float32).reshape(k, 4)
    bench.dump_outputs(str(tmp_path), cent, maps, [0, 1], n_band, 2 * n_band, k)
    d = _load(str(tmp_path))
    assert set(d) == {"centroids", "label_counts", "labels_sample_index", "labels_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    full = torch.cat(maps).numpy()
    assert np.array_equal(d["centroids"], cent)
    assert np.array_equal(d["labels_sample_index"], np.arange(2 * n_band))
    assert np.array_equal(d["labels_sample"], full.astype(np.float32))
    assert np.array_equal(d["label_counts"], np.bincount(full, minlength=k))


def test_sample_is_seeded_and_gathered_ranks_match_one_process(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LABEL_SAMPLE", 5000)
    k, n_band, world = 64, 4096, 3
    maps = _maps(k, n_band, world)
    cent = np.ones((k, 4), np.float32)
    one, again, ranks = (str(tmp_path / n) for n in ("one", "again", "ranks"))
    bench.dump_outputs(one, cent, maps, list(range(world)), n_band, world * n_band, k)
    bench.dump_outputs(again, cent, maps, list(range(world)), n_band, world * n_band, k)
    # ranks 1 and 2 hand their pieces to the gather; rank 0 collects everything and writes
    sent = []
    for r in (1, 2):
        bench.dump_outputs(ranks, None, [maps[r]], [r], n_band, world * n_band, k, gather=lambda obj: sent.append(obj) or ([], []))
    assert not os.path.exists(ranks)
    gather = lambda obj: ([obj[0]] + [s[0] for s in sent], [obj[1]] + [s[1] for s in sent])
    bench.dump_outputs(ranks, cent, [maps[0]], [0], n_band, world * n_band, k, gather=gather)
    a, b, c = _load(one), _load(again), _load(ranks)
    for name in a:
        assert np.array_equal(a[name], b[name]) and np.array_equal(a[name], c[name]), name
    idx = a["labels_sample_index"].astype(np.int64)
    assert idx.shape == (5000,) and np.all(np.diff(idx) >= 0) and idx[0] >= 0 and idx[-1] < world * n_band
    full = torch.cat(maps).numpy()
    assert np.array_equal(a["labels_sample"], full[idx].astype(np.float32))
    assert np.array_equal(a["label_counts"], np.bincount(full, minlength=k))


def test_dump_of_the_headline_stays_under_64_mb():
    k = bench.K
    per_sample = np.dtype(np.float64).itemsize + np.dtype(np.float32).itemsize      # index + label
    total = bench.DUMP_LABEL_SAMPLE * per_sample + k * 4 * 4 + k * 8
    assert bench.WIDTH * bench.ROWS_PER_GPU > bench.DUMP_LABEL_SAMPLE and total < 64 * 2 ** 20
