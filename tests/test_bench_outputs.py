"""bench.py's --dump-outputs and --full: the dumped arrays (dtype, size limit, the fixed row
sample of a frame over the limit), and on the GPU one plain run from the command line: its
result line, and its dumped framebuffer against the oracle's frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_whole_small_arrays(tmp_path):
    d = str(tmp_path / "out")
    fb = torch.arange(7 * 5 * 3, dtype=torch.float32).reshape(7, 5, 3)
    u8 = (torch.arange(7 * 5 * 3) % 251).to(torch.uint8).reshape(7, 5, 3)
    f64 = torch.linspace(0, 1, 12, dtype=torch.float64).reshape(4, 3)
    written = bench.dump_outputs(d, {"framebuffer": fb, "frame_rgb8": u8, "depth": f64})
    assert sorted(os.listdir(d)) == ["depth.npy", "frame_rgb8.npy", "framebuffer.npy"] == sorted(written)
    a, b, c = (np.load(os.path.join(d, n + ".npy")) for n in ("framebuffer", "frame_rgb8", "depth"))
    assert a.dtype == np.float32 and np.array_equal(a, fb.numpy())
    assert b.dtype == np.float32 and np.array_equal(b, u8.numpy().astype(np.float32))
    assert c.dtype == np.float64 and np.array_equal(c, f64.numpy())
    assert written["framebuffer.npy"] == [7, 5, 3]


def test_dump_samples_rows_of_a_frame_over_the_limit(tmp_path, monkeypatch):
    """Over the limit: an ascending row sample that is the same in every run, its indices
    beside it, and all files together within the limit."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 40000)
    rs = np.random.RandomState(3)
    fb = torch.from_numpy(rs.rand(101, 37, 3).astype(np.float32))  # 44,844 B: over; odd sizes
    small = torch.from_numpy(rs.rand(9, 37, 3).astype(np.float32))
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, {"framebuffer": fb, "small": small})
    bench.dump_outputs(d2, {"framebuffer": fb, "small": small})
    assert sorted(os.listdir(d1)) == ["framebuffer.npy", "framebuffer_rows.npy", "small.npy"]
    assert dir_bytes(d1) <= 40000
    rows = np.load(os.path.join(d1, "framebuffer_rows.npy"))
    x = np.load(os.path.join(d1, "framebuffer.npy"))
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < 101
    # its share of the limit is half (two arrays): at least a third of the frame's rows fit
    assert 34 <= len(rows) < 101 and x.shape == (len(rows), 37, 3)
    assert np.array_equal(x, fb.numpy()[rows.astype(np.int64)])
    assert np.array_equal(np.load(os.path.join(d1, "small.npy")), small.numpy())
    for n in os.listdir(d1):
        assert np.array_equal(np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n)))


def test_dump_of_the_largest_config_stays_under_64_mb():
    """The row sample's size for DepthOfField 4K (3840x2160 fp32 RGB, 99.5 MB), without writing it."""
    assert bench.DUMP_BYTES == 64 * 10 ** 6
    row = 3840 * 3 * 4
    fit = (bench.DUMP_BYTES - 1024) // (row + 8)
    assert 0 < fit < 2160 and fit * (row + 8) + 1024 <= bench.DUMP_BYTES


def test_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "x"


FULL_ONLY = ("frame_ms", "rgb8", "roofline", "segments_per_frame", "cast_rays_per_frame", "shadow_rays_per_frame",
             "cpu_baseline", "cpu_baseline_native")


@pytest.mark.gpu
def test_plain_run_result_line_and_dump(tmp_path):
    """One plain run: the line has the value's fields and none of --full's, --steps sets the
    timed steps, and the dumped framebuffer is the oracle's frame bit for bit."""
    from oracle import oracle as O
    d = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--clock-warmup-s", "0", "--dump-outputs", d],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["metric"] == bench.METRIC and r["unit"] == "Mrays/s" and r["higher_is_better"] is True
    assert r["dtype"] == "fp32 vectors + fp64 scalars (reference numerics)"
    assert (r["steps"], r["warmup"], r["n_gpus"], r["full"]) == (3, 1, 1, False)
    assert r["ms_per_step"] > 0
    # value = samples per step / ms_per_step (both rounded in the line: 5 decimals of ms_per_step)
    assert r["value"] == pytest.approx(1920 * 1080 / r["ms_per_step"] / 1e3, rel=0.5e-5 / r["ms_per_step"] + 1e-6)
    assert not [k for k in FULL_ONLY if k in r]
    assert sorted(os.listdir(d)) == ["framebuffer.npy"] and r["dumped"] == {"framebuffer.npy": [1080, 1920, 3]}
    fb = np.load(os.path.join(d, "framebuffer.npy"))
    assert fb.dtype == np.float32 and fb.shape == (1080, 1920, 3)
    sd, base = bench.scene_dict("tsp1080")
    ref = O.OracleScene(sd, base).render()  # float64 [column, row from the bottom]; the framebuffer is [row, column]
    assert np.array_equal(fb.astype(np.float64), np.transpose(ref, (1, 0, 2))[::-1])
