"""bench.py's plain run and --dump-outputs on the CPU: the options, and that the dump holds the visible samples of the output planes
(padding left out, the seeded sample where the batch is larger than the budget).  tests/test_bench_dist.py runs the dump on the GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_a_plain_run_is_the_default():
    a = bench.parse_args([])
    assert not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--steps", "7", "--warmup", "0"])
    assert a.full and a.dump_outputs == "out" and a.steps == 7 and a.warmup == 0
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def _device_batch(torch, fmt, ddims, frames, shift, seed=7):
    """Output tensors laid out as make_workload lays them out (256-byte rows, one spare row per frame with a shift)."""
    rng = np.random.default_rng(seed)
    sb = fmt.sample_bytes
    out = []
    for (w, h) in ddims:
        pitch = (w * sb + 255) // 256 * 256 // sb
        shape = (frames, h + (1 if shift else 0), pitch)
        a = rng.random(shape, dtype=np.float32) if sb == 4 else rng.integers(0, 1 << fmt.bits, shape).astype(fmt.dtype)
        out.append(torch.from_numpy(a))
    return out


def _visible(t, w, h, shift_elems):
    """(frames, h, w) view of the visible samples, rows starting shift_elems samples into the tensor."""
    a = t.numpy()
    flat = a.reshape(-1)[shift_elems:]
    return np.lib.stride_tricks.as_strided(flat, (a.shape[0], h, w), a.strides)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("budget", [None, 1 << 14], ids=["whole", "sample"])
@pytest.mark.parametrize("fmt_name", ["Y8", "YUV420P16", "RGBPS"])
def test_the_dump_holds_the_visible_samples(pkg, monkeypatch, tmp_path, fmt_name, budget, shift):
    import torch
    monkeypatch.setattr(bench, "through_pinned_to_device", lambda torch, t: t)
    monkeypatch.setattr(bench, "through_pinned_to_host", lambda torch, t: t.clone())
    if budget:
        monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    fmt = pkg.FORMATS[fmt_name]
    ddims = fmt.plane_dims(70, 38)
    frames = 5
    dst = _device_batch(torch, fmt, ddims, frames, shift)
    bench.dump_outputs(torch, str(tmp_path), dst, ddims, fmt, shift * fmt.sample_bytes)
    sizes = [frames * w * h for (w, h) in ddims]
    files = sorted(os.listdir(tmp_path))
    total = 0
    for i, (t, (w, h)) in enumerate(zip(dst, ddims)):
        want = _visible(t, w, h, shift).astype(np.float32)
        if budget is None:
            assert files[i] == f"plane{i}.npy"
            got = np.load(tmp_path / files[i])
            assert got.dtype == np.float32 and got.shape == (frames, h, w)
            assert np.array_equal(got, want)
        else:
            assert files[i] == f"plane{i}_sample.npy"
            got = np.load(tmp_path / files[i])
            n = budget // 4 * sizes[i] // sum(sizes)
            pos = bench.dump_positions(frames, w, h, n)
            assert np.array_equal(pos, bench.dump_positions(frames, w, h, n))    # the same positions every run
            assert len(pos) == n and pos[0] >= 0 and pos[-1] < sizes[i] and np.all(np.diff(pos) >= 0)
            assert got.dtype == np.float32 and np.array_equal(got, want.reshape(-1)[pos])
        total += got.nbytes
    assert len(files) == len(ddims) and total <= bench.DUMP_BUDGET_BYTES


def test_the_headline_batch_is_dumped_as_a_sample_within_64_mb(pkg):
    """C2 at 1024 frames holds 8.5 G output samples: the sample of it stays under 64 MB with the .npy headers."""
    fmt_name, sw, sh, dw, dh, _, frames = bench.CONFIGS["C2"]
    ddims = pkg.FORMATS[fmt_name].plane_dims(dw, dh)
    sizes = [frames * w * h for (w, h) in ddims]
    budget = bench.DUMP_BUDGET_BYTES // 4
    assert sum(sizes) > budget
    assert sum(budget * s // sum(sizes) for s in sizes) * 4 + 128 * len(sizes) <= 64_000_000
