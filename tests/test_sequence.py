"""Frame sequences without a GPU: the windows rtx.frame_windows makes, what
Scene.render_sequence refuses, the sequence camera's descriptor (rtx_camera_desc.n_frames),
the C entry points' argument checks, and the CLI's arguments and file names."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import rtx
from rtx import _native as N
from rtx import main as cli
from rtx.scene import sequence_windows


def test_frame_windows_values():
    # one time per frame: t_f = start + (stop - start) / frames * f, in Python floats
    assert rtx.frame_windows(0.0, 2.0, 5) == [[0.0 + 2.0 / 5 * f] for f in range(5)]
    assert rtx.frame_windows(-4, 4, 4) == [[-4.0], [-2.0], [0.0], [2.0]]
    # a shutter: set_motion's rule ([dt * i] + [time] * final) shifted to the frame's start
    w = rtx.frame_windows(1.0, 4.0, 3, shutter=0.5, samples=2, final=1)
    assert w == [[1.0, 1.25, 1.5], [2.0, 2.25, 2.5], [3.0, 3.25, 3.5]]
    start, stop, frames, shutter, samples = 0.1, 0.7, 7, 0.3, 3
    got = rtx.frame_windows(start, stop, frames, shutter, samples, final=2)
    for f in range(frames):
        t = start + (stop - start) / frames * f
        assert got[f] == [t + shutter / samples * i for i in range(samples)] + [t + shutter] * 2
    # the first window of a sequence from 0 is the camera's own set_motion table
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 8))
    vc = sc.vc
    times = list(vc.motion_times)
    vc.set_motion(0.75, 4, 1)
    assert rtx.frame_windows(0.0, 3.0, 2, shutter=0.75, samples=4, final=1)[0] == list(vc.motion_times)
    vc.motion_times = times
    # only final samples: every time of the window is the shutter's end
    assert rtx.frame_windows(0.0, 1.0, 2, shutter=0.25, samples=0, final=2) == [[0.25, 0.25], [0.75, 0.75]]
    assert all(type(t) is float for w in rtx.frame_windows(0, 1, 3) for t in w)


@pytest.mark.parametrize("args", [(0, 1, 0), (0, 1, 2, 0.0, 0, 0), (0, 1, 2, 0.0, -1, 2), (0, 1, 2, 0.0, 1, -1),
                                  (0, float("inf"), 2), (float("nan"), 1, 2), (0, 1, 2, float("inf"))])
def test_frame_windows_refuses(args):
    with pytest.raises(ValueError):
        rtx.frame_windows(*args)


def test_sequence_windows_normalises_and_refuses():
    assert sequence_windows([0, 0.5, 1]) == [[0.0], [0.5], [1.0]]  # a flat list: T = 1
    assert sequence_windows(np.array([[0.0, 1.0], [2.0, 3.0]])) == [[0.0, 1.0], [2.0, 3.0]]
    assert sequence_windows(((0, 1), (2, 3))) == [[0.0, 1.0], [2.0, 3.0]]
    for bad in ([], [[]], [[0.0, 1.0], [2.0]], [[0.0], [math.nan]], [[0.0], [math.inf]], [0.0, [1.0]], 3.0, None,
                [[0.0], []]):
        with pytest.raises(ValueError):
            sequence_windows(bad)


def test_render_sequence_refuses_bad_windows_before_any_gpu_call():
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 8))
    for bad in ([], [[0.0, 1.0], [2.0]], [[math.nan]], [math.inf, 0.0]):
        with pytest.raises(ValueError):
            sc.render_sequence(bad)
    with pytest.raises(ValueError):
        sc.render_sequence([0.0, 1.0], batch=0)
    with pytest.raises(ValueError):
        sc.render_sequence([0.0, 1.0], frames=(1, 2))
    assert sc._native is None  # nothing was uploaded


def test_sequence_camera_desc():
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(24, 16))
    d0, t0 = sc.camera_desc()
    assert d0.n_frames == 0 and d0.n_times == len(sc.vc.motion_times)
    assert list(t0["times"]) == list(sc.vc.motion_times)
    windows = rtx.frame_windows(0.0, 2.0, 4, shutter=0.3, samples=2, final=1)
    d, t = sc.camera_desc(windows=windows)
    assert (d.n_frames, d.n_times) == (4, 3)                    # n_times stays the per-frame window length
    assert [d.times[i] for i in range(12)] == [x for w in windows for x in w]  # [F][T] order
    assert t["times"].dtype == np.float64 and t["times"].shape == (12,)
    # everything else is the ordinary camera's
    for f in ("width", "height", "col0", "ncols", "d", "focal_length", "n_dof", "n_aa", "jitter", "jitter_scale",
              "seed"):
        assert getattr(d, f) == getattr(d0, f), f
    assert list(sc.vc.motion_times) == list(t0["times"])        # the camera's own times are not touched
    d1, _ = sc.camera_desc(windows=[0.25, 0.5])
    assert (d1.n_frames, d1.n_times, d1.times[0], d1.times[1]) == (2, 1, 0.25, 0.5)
    with pytest.raises(ValueError):
        sc.camera_desc(windows=[[0.0, 1.0], [2.0]])


def test_sequence_is_part_of_the_camera_key(monkeypatch):
    """A sequence upload is keyed by its windows, so the same sequence is uploaded once and a
    later render() finds another key and uploads the ordinary camera again."""
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 8))
    calls = []
    monkeypatch.setattr(sc, "native", lambda: types.SimpleNamespace(h=None))
    monkeypatch.setattr(N, "call", lambda fn, *a: calls.append(fn))
    w = sequence_windows([0.0, 1.0])
    sc._set_camera(0, 1, w)
    sc._set_camera(0, 1, sequence_windows([0.0, 1.0]))
    assert calls == ["rtx_camera_set"]
    sc._set_camera(0, 1, sequence_windows([0.0, 1.5]))
    sc._set_camera(0, 1)
    sc._set_camera(0, 1)
    sc._set_camera(0, 1, w)
    assert calls == ["rtx_camera_set"] * 4


def test_sequence_entry_points_check_arguments_without_gpu():
    lib = N.load()
    assert lib.rtx_abi_version() == 6
    for fn in ("rtx_render_sequence", "rtx_render_groups_sequence"):
        assert getattr(lib, fn)(None, 0, 1, None, 0, 0, 1, 0, None, None) == N.RTX_ERR_INVALID
        assert fn.encode() + b": null scene" in lib.rtx_last_error()
        assert getattr(lib, fn)(None, 0, 1, None, 0, -1, 1, 0, None, None) == N.RTX_ERR_INVALID
        assert b"frame0" in lib.rtx_last_error()
    assert C.sizeof(N.rtx_camera_desc) % 8 == 0 and N.rtx_camera_desc.n_frames.offset > N.rtx_camera_desc.noise.offset


def test_cli_frame_names():
    assert cli.frame_names("out.png", 3) == ["out_0000.png", "out_0001.png", "out_0002.png"]
    assert cli.frame_names("a/b.c/frames", 2) == ["a/b.c/frames_0000", "a/b.c/frames_0001"]
    assert cli.frame_names("f%03d.png", 2) == ["f000.png", "f001.png"]
    assert cli.frame_names("x%d.png", 12)[11] == "x11.png"
    assert len(set(cli.frame_names("out.png", 12000))) == 12000  # (more than four digits still differ)


def test_cli_sequence_arguments(capsys):
    a = cli.parse(["--infile", "s.json", "--frames", "8", "--time-range", "-1", "3", "--shutter", "0.2",
                   "--shutter-samples", "4", "--outfile", "o%02d.png"])
    assert (a.frames, a.time_range, a.shutter, a.shutter_samples) == (8, [-1.0, 3.0], 0.2, 4)
    a = cli.parse(["--infile", "s.json", "--frames", "2"])
    assert (a.frames, a.time_range, a.shutter, a.shutter_samples, a.outfile) == (2, None, 0.0, 1, "out.png")
    assert cli.parse(["--infile", "s.json"]).frames is None       # the ordinary render is unchanged
    for bad, word in ((["--frames", "2", "--distributed"], "--distributed"),
                      (["--frames", "2", "--subimage", "0", "--tasks", "2"], "--subimage"),
                      (["--frames", "2", "--subimage", "1"], "--subimage"),
                      (["--frames", "0"], ">= 1"), (["--frames", "2", "--shutter-samples", "0"], ">= 1"),
                      (["--frames", "2", "--outfile", "a%d_%d.png"], "pattern"),
                      (["--time-range", "0", "1"], "need --frames"), (["--shutter", "0.5"], "need --frames")):
        with pytest.raises(SystemExit):
            cli.parse(["--infile", "s.json"] + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_renders_the_sequence_in_batches(tmp_path, monkeypatch):
    """render_frames_to_files: the default time range is 0 .. the scene's last motion time,
    the frames go through render_sequence's uint8 path in bounded batches, one PNG each."""
    import torch
    from PIL import Image
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(6, 4))
    last = float(sc.vc.motion_times[-1])
    assert last > 0.0
    seen = []

    def fake(windows, rgb8=False, **kw):
        assert rgb8 is True and not kw
        seen.append(windows)
        return torch.stack([torch.full((4, 6, 3), len(seen) * 10 + k, dtype=torch.uint8) for k in range(len(windows))])
    monkeypatch.setattr(sc, "render_sequence", fake)
    monkeypatch.setattr(cli, "SEQUENCE_BATCH_FRAMES", 2)
    args = cli.parse(["--infile", "s.json", "--frames", "5", "--shutter", "0.1", "--shutter-samples", "2",
                      "--outfile", str(tmp_path / "f.png")])
    names = cli.render_frames_to_files(sc, args)
    assert [len(w) for w in seen] == [2, 2, 1]
    assert [t for w in seen for t in w] == rtx.frame_windows(0.0, last, 5, 0.1, 2)
    assert names == [str(tmp_path / ("f_%04d.png" % f)) for f in range(5)]
    for f, n in enumerate(names):
        assert np.asarray(Image.open(n)).tolist() == np.full((4, 6, 3), (f // 2 + 1) * 10 + f % 2).tolist()
    monkeypatch.setattr(cli, "SEQUENCE_BATCH_BYTES", 6 * 4 * 3)   # one frame's bytes: one frame per batch
    seen.clear()
    args = cli.parse(["--infile", "s.json", "--frames", "3", "--time-range", "1", "2", "--outfile",
                      str(tmp_path / "g%d.png")])
    assert cli.render_frames_to_files(sc, args) == [str(tmp_path / ("g%d.png" % f)) for f in range(3)]
    assert seen == [[[1.0]], [[1.0 + 1.0 / 3]], [[1.0 + 1.0 / 3 * 2]]]
