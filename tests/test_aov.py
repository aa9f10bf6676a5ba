"""First-hit feature buffers without a GPU: the C entry point's export and argument checks,
what Scene.render_aovs and Scene.pick refuse before any upload, and the CLI's arguments and
.npz writer."""
import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from rtx import main as cli


def test_entry_point_is_exported_and_the_abi_is_unchanged():
    lib = N.load()
    assert lib.rtx_abi_version() == 6 and N.ABI_VERSION == 6
    assert "rtx_render_aov" in N.EXPORTS and hasattr(lib, "rtx_render_aov")
    assert len(lib.rtx_render_aov.argtypes) == 11
    assert rtx.AOV_NAMES == ("depth", "normal", "position", "albedo", "object", "material")


def test_entry_point_checks_arguments_without_gpu():
    lib = N.load()
    assert lib.rtx_render_aov(None, 0, 1, 0, None, None, None, None, None, None, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_aov: null scene" in lib.rtx_last_error()
    # (a null scene is refused whatever else is passed)
    assert lib.rtx_render_aov(None, -1, -1, -1, 16, 16, 16, 16, 16, 16, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_aov: null scene" in lib.rtx_last_error()


def _cpu_out(shape, dtype):
    return torch.zeros(shape, dtype=dtype)


def test_render_aovs_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    for bad in (("colour",), ("depth", "colour"), (), [], "rgb", ("depth", "depth")):
        with pytest.raises(ValueError):
            sc.render_aovs(bad)
    for kw in (dict(frame=1), dict(frame=-1), dict(windows=[0.0, 1.0], frame=2), dict(windows=[0.0, 1.0], frame=-1),
               dict(windows=[]), dict(windows=[[0.0, 1.0], [2.0]]), dict(row0=-1), dict(row0=4, nrows=3),
               dict(nrows=-1), dict(row0=7)):
        with pytest.raises(ValueError):
            sc.render_aovs(**kw)
    with pytest.raises(IndexError):  # (strip_columns, as render() raises it)
        sc.render_aovs(subimage=2, tasks=2)
    # out: a tensor per requested name, contiguous, on the device, of the buffer's shape and type
    bad_out = (
        dict(depth=_cpu_out((6, 8), torch.float32)),                      # not on the device
        dict(normal=_cpu_out((6, 8), torch.float32)),                     # and not [H, W, 3]
        dict(object=_cpu_out((6, 8), torch.float32)),                     # and not int32
        dict(depth=np.zeros((6, 8), np.float32)),                         # not a tensor
        dict(colour=_cpu_out((6, 8, 3), torch.float32)),                  # an unknown name
    )
    for out in bad_out:
        with pytest.raises(ValueError):
            sc.render_aovs(out=out)
    with pytest.raises(ValueError):  # a buffer that was not requested
        sc.render_aovs(("depth",), out=dict(object=_cpu_out((6, 8), torch.int32)))
    assert sc._native is None  # nothing was uploaded


def test_pick_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(8, 6))
    for col, row in ((-1, 0), (8, 0), (0, 6), (0, -1)):
        with pytest.raises(ValueError):
            sc.pick(col, row)
    with pytest.raises(ValueError):
        sc.pick(4, 0, subimage=1, tasks=2)   # the second strip holds columns 0..3
    with pytest.raises(ValueError):
        sc.pick(0, 0, frame=1)
    with pytest.raises(ValueError):
        sc.pick(0, 0, aovs=("depth",))       # not a camera argument
    assert sc._native is None


def test_cli_aov_arguments(capsys):
    a = cli.parse(["--infile", "s.json", "--aovs", "o.npz"])
    assert (a.aovs, a.aov_names, a.outfile) == ("o.npz", None, "out.png")
    a = cli.parse(["--infile", "s.json", "--aovs", "o.npz", "--aov-names", "depth", "object"])
    assert a.aov_names == ["depth", "object"]
    a = cli.parse(["--infile", "s.json", "--aovs", "o.npz", "--subimage", "1", "--tasks", "2"])
    assert (a.aovs, a.subimage, a.tasks) == ("o.npz", 1, 2)
    a = cli.parse(["--infile", "s.json"])
    assert a.aovs is None and a.aov_names is None                  # the ordinary render is unchanged
    for bad, word in ((["--aovs", "o.npz", "--distributed"], "--distributed"),
                      (["--aovs", "o.npz", "--frames", "2"], "--frames"),
                      (["--aovs", "o.npz", "--aov-names", "colour"], "--aov-names"),
                      (["--aovs", "o.npz", "--aov-names", "depth", "depth"], "--aov-names"),
                      (["--aov-names", "depth"], "--aovs")):
        with pytest.raises(SystemExit):
            cli.parse(["--infile", "s.json"] + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_writes_the_chosen_buffers(tmp_path, monkeypatch):
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(6, 4))
    seen = []

    def fake(aovs, **kw):
        seen.append((tuple(aovs), kw))
        return {n: torch.full((4, 6, 3) if n in ("normal", "position", "albedo") else (4, 6), k + 1,
                              dtype=torch.int32 if n in ("object", "material") else torch.float32)
                for k, n in enumerate(aovs)}
    monkeypatch.setattr(sc, "render_aovs", fake)
    path = str(tmp_path / "buffers")                               # (the name is kept as given)
    args = cli.parse(["--infile", "s.json", "--aovs", path, "--aov-names", "object", "normal"])
    assert cli.write_aovs(sc, args) == path
    with np.load(path) as z:
        assert sorted(z.files) == ["normal", "object"]
        assert z["object"].dtype == np.int32 and z["object"].tolist() == np.full((4, 6), 1).tolist()
        assert z["normal"].dtype == np.float32 and z["normal"].shape == (4, 6, 3) and (z["normal"] == 2).all()
    args = cli.parse(["--infile", "s.json", "--aovs", str(tmp_path / "all.npz"), "--subimage", "1", "--tasks", "3"])
    cli.write_aovs(sc, args)
    with np.load(str(tmp_path / "all.npz")) as z:
        assert sorted(z.files) == sorted(rtx.AOV_NAMES)
    assert seen == [(("object", "normal"), {}), (rtx.AOV_NAMES, dict(subimage=1, tasks=3))]
