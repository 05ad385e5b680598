"""bench.py --dump-outputs on CPU tensors: the files are float32 / float64, stay under 64 MB, sample the same rows every run and
hold the slot bytes up to each block's size and zeros past it."""
import importlib.util
import os

import numpy as np
import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dump(bench, d, nb, stride):
    g = torch.Generator().manual_seed(nb)
    dig = torch.randint(0, 256, (nb, 64), dtype=torch.uint8, generator=g)
    sizes = torch.randint(0, stride, (nb,), dtype=torch.int32, generator=g)
    dst = torch.randint(0, 256, (nb * stride,), dtype=torch.uint8, generator=g)
    totals = torch.tensor([123456789012, 5], dtype=torch.int64)
    bench.dump_outputs(str(d), torch, dig, totals, dst, stride, sizes, nb)
    return dig.numpy(), sizes.numpy(), dst.numpy()


def test_dump_outputs_sampled_and_exact(tmp_path):
    bench = _bench()
    nb, stride = 3 << 20, 16          # more blocks than every budget: all three arrays are sampled
    dig, sizes, dst = _dump(bench, tmp_path / "a", nb, stride)
    _dump(bench, tmp_path / "b", nb, stride)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["digests.npy", "digests_rows.npy", "payload.npy", "payload_rows.npy",
                                                           "sizes.npy", "sizes_rows.npy", "totals.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) < 64 << 20
    load = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    for f in names:
        assert load[f[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(load[f[:-4]], np.load(tmp_path / "b" / f)), f
    rows = {k: load[k + "_rows"].astype(np.int64) for k in ("digests", "sizes", "payload")}
    assert np.array_equal(load["digests"], dig[rows["digests"]])
    assert np.array_equal(load["sizes"], sizes[rows["sizes"]])
    slots = dst.reshape(nb, stride)[rows["payload"]]
    z = sizes[rows["payload"]]
    assert np.array_equal(load["payload"], np.where(np.arange(stride)[None, :] < z[:, None], slots, 0))
    assert load["totals"].tolist() == [123456789012, 5]


def test_dump_outputs_small_batch_whole(tmp_path):
    bench = _bench()
    nb, stride = 70, 65824
    dig, sizes, dst = _dump(bench, tmp_path, nb, stride)
    assert np.array_equal(np.load(tmp_path / "digests.npy"), dig)
    assert np.array_equal(np.load(tmp_path / "sizes.npy"), sizes)
    assert np.load(tmp_path / "payload.npy").shape == (63, stride)     # 4 Mi bytes of slots
    assert not os.path.exists(tmp_path / "digests_rows.npy") and not os.path.exists(tmp_path / "sizes_rows.npy")
