"""bench.py --dump-outputs without a GPU: `dump_outputs` on host tensors shaped like the C3 step's
outputs (grid in the reference memory order, point gradients, per-pose scalars)."""
import os

import numpy as np
import torch

import bench


def _c3_like_outputs(seed):
    g = torch.Generator().manual_seed(seed)
    P = 10_000_000
    out = torch.rand((256, 256, 256), generator=g).permute(2, 1, 0)  # [i1, i2, i3] view
    rot = torch.rand((1, 3, 3), generator=g).transpose(1, 2)[0]
    return {"out": out, "ds_dpoints": torch.rand((P, 3), generator=g),
            "ds_drotation": rot, "ds_dtranslation": torch.rand(3, generator=g),
            "ds_dbackground": torch.rand((), generator=g), "ds_dout_weight": torch.rand((), generator=g),
            "ds_dpoint_weight": torch.rand(P, generator=g, dtype=torch.float64), "unused": None}


def test_dump_outputs_stays_within_64_mb_and_samples_reproducibly(tmp_path):
    arrays = _c3_like_outputs(0)
    m1 = bench.dump_outputs(str(tmp_path / "a"), arrays)
    m2 = bench.dump_outputs(str(tmp_path / "b"), _c3_like_outputs(0))
    assert m1 == m2 and "unused" not in m1
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{n}.npy" for n in arrays if n != "unused")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    # small outputs whole, with their shape and values
    for n in ("ds_drotation", "ds_dtranslation", "ds_dbackground", "ds_dout_weight"):
        assert "sample" not in m1[n]
        got = np.load(tmp_path / "a" / f"{n}.npy")
        assert got.shape == tuple(arrays[n].shape), n
        np.testing.assert_array_equal(got, arrays[n].numpy())
    # large ones: the documented sample of the memory-order elements
    for n in ("out", "ds_dpoints", "ds_dpoint_weight"):
        assert "sample" in m1[n] and m1[n]["shape"] == list(arrays[n].shape)
        s, t = m1[n]["sample"], arrays[n]
        idx = np.unique(np.random.default_rng(s["seed"]).integers(0, t.numel(), size=s["draws"]))
        got = np.load(tmp_path / "a" / f"{n}.npy")
        assert got.ndim == 1 and got.size == s["elements"] == idx.size
        np.testing.assert_array_equal(got, bench._memory_order_flat(t).numpy()[idx])
    # the grid is sampled from its storage order: element 0 of storage is out[0, 0, 0], element 1 out[1, 0, 0]
    flat = bench._memory_order_flat(arrays["out"])
    assert flat[1] == arrays["out"][1, 0, 0] and flat[256] == arrays["out"][0, 1, 0]
