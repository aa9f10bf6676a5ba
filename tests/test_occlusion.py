"""Occlusion buffers without a GPU: the C entry point's export and argument checks, what
Scene.render_occlusion refuses before any upload, rtx.cosine_directions, the CLI's arguments
and .npz writer, and the numpy restatement of the orthonormal frame (tests/occref.py)."""
import copy

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from rtx import main as cli
from rtx.helperclasses import _sunflower_terms
import occref

f32 = np.float32


def test_entry_point_is_exported_and_the_abi_is_unchanged():
    lib = N.load()
    assert lib.rtx_abi_version() == 6 and N.ABI_VERSION == 6
    assert "rtx_render_occlusion" in N.EXPORTS and hasattr(lib, "rtx_render_occlusion")
    assert len(lib.rtx_render_occlusion.argtypes) == 10
    assert N.RTX_AO_MAX_DIRS == 64
    assert rtx.OCCLUSION_NAMES == ("lights", "ao")


def test_entry_point_checks_arguments_without_gpu():
    lib = N.load()
    assert lib.rtx_render_occlusion(None, 0, 1, 0, None, None, None, 0, 1.0, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_occlusion: null scene" in lib.rtx_last_error()
    # (a null scene is refused whatever else is passed)
    dirs = (N.C.c_float * 3)(0.0, 0.0, 1.0)
    assert lib.rtx_render_occlusion(None, -1, -1, -1, 16, 16, dirs, 1, float("nan"), None) == N.RTX_ERR_INVALID
    assert b"rtx_render_occlusion: null scene" in lib.rtx_last_error()


def _many_lights(n):
    from rtx.io import bundled_scene_dict
    d = bundled_scene_dict("TwoSpheresPlane", resolution=(8, 6))
    d["lights"] = [dict(copy.deepcopy(d["lights"][0]), name="p%d" % i) for i in range(n)]
    return rtx.load_scene(d, verbose=False)


def test_render_occlusion_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    for bad in (("depth",), ("lights", "depth"), (), [], "shadow", ("ao", "ao")):
        with pytest.raises(ValueError):
            sc.render_occlusion(bad)
    for kw in (dict(frame=1), dict(frame=-1), dict(windows=[0.0, 1.0], frame=2), dict(windows=[0.0, 1.0], frame=-1),
               dict(windows=[]), dict(windows=[[0.0, 1.0], [2.0]]), dict(row0=-1), dict(row0=4, nrows=3),
               dict(nrows=-1), dict(row0=7),
               dict(ao_samples=0), dict(ao_samples=65), dict(ao_samples=-1), dict(ao_samples=2.5), dict(ao_samples=True),
               dict(ao_radius=0.0), dict(ao_radius=-1.0), dict(ao_radius=float("nan")), dict(ao_radius=-float("inf")),
               dict(ao_radius="far"),
               dict(ao_dirs=np.zeros((0, 3))), dict(ao_dirs=np.zeros((65, 3))), dict(ao_dirs=np.zeros((4, 2))),
               dict(ao_dirs=np.zeros(3)), dict(ao_dirs=[[0.0, 0.0, float("nan")]]),
               dict(ao_dirs=[[0.0, float("inf"), 1.0]]), dict(ao_dirs=[[1e39, 0.0, 1.0]]),  # (inf as fp32)
               dict(ao_dirs="up")):
        with pytest.raises(ValueError):
            sc.render_occlusion(**kw)
    with pytest.raises(IndexError):  # (strip_columns, as render() raises it)
        sc.render_occlusion(subimage=2, tasks=2)
    # the ambient-occlusion arguments are not looked at when "ao" is not asked for
    # (the call then fails later, on the out tensor)
    with pytest.raises(ValueError, match="out"):
        sc.render_occlusion("lights", ao_samples=0, ao_radius=-1.0, out=dict(lights=torch.zeros((6, 8))))
    bad_out = (
        dict(ao=torch.zeros((6, 8), dtype=torch.float32)),                  # not on the device
        dict(lights=torch.zeros((6, 8), dtype=torch.int32)),                # not on the device
        dict(lights=torch.zeros((6, 8), dtype=torch.float32)),              # and not int32
        dict(ao=torch.zeros((6, 8, 3), dtype=torch.float32)),               # and not [H, W]
        dict(ao=np.zeros((6, 8), np.float32)),                              # not a tensor
        dict(depth=torch.zeros((6, 8), dtype=torch.float32)),               # an unknown name
    )
    for out in bad_out:
        with pytest.raises(ValueError):
            sc.render_occlusion(out=out)
    with pytest.raises(ValueError):  # a buffer that was not requested
        sc.render_occlusion(("ao",), out=dict(lights=torch.zeros((6, 8), dtype=torch.int32)))
    assert sc._native is None  # nothing was uploaded


def test_more_than_32_lights_are_refused_for_the_mask_only():
    sc = _many_lights(33)
    with pytest.raises(ValueError, match="32 lights"):
        sc.render_occlusion()
    with pytest.raises(ValueError, match="32 lights"):
        sc.render_occlusion("lights")
    # "ao" alone passes the light check (and fails on its out tensor, still before any upload)
    with pytest.raises(ValueError, match="out"):
        sc.render_occlusion("ao", out=dict(ao=torch.zeros((6, 8))))
    with pytest.raises(ValueError, match="out"):
        _many_lights(32).render_occlusion(out=dict(ao=torch.zeros((6, 8))))
    assert sc._native is None


@pytest.mark.parametrize("k", [1, 2, 7, 16, 64])
def test_cosine_directions(k):
    d = rtx.cosine_directions(k)
    assert d.dtype == np.float32 and d.shape == (k, 3)
    # the fp64-then-round definition: the sunflower disk points, z from them, one rounding
    sq, co, si, sn = _sunflower_terms(k)
    x, y = sq / sn * co, sq / sn * si
    z = np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y))
    assert np.array_equal(d, np.stack([x, y, z], axis=1).astype(np.float32))
    assert (d[:, 2] >= 0).all()
    # unit length: the fp64 vector is unit to a few fp64 ulps, each component is then rounded
    # once (relative error 2^-24), so the length is off by at most 2^-24 (1 + a few 2^-29)
    length = np.sqrt((d.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 2.0 ** -23
    # the radii grow: z falls from the pole to the rim, whose point lies on the unit circle
    assert (np.diff(d[:, 2]) < 0).all() if k > 1 else True
    assert d[-1, 2] < 1e-7 and abs(np.hypot(float(d[-1, 0]), float(d[-1, 1])) - 1.0) < 1e-7


def test_cosine_directions_arguments():
    one = rtx.cosine_directions(1)
    assert one.shape == (1, 3) and abs(np.hypot(float(one[0, 0]), float(one[0, 1])) - 1.0) < 1e-7  # the rim point
    for bad in (0, -3):
        with pytest.raises(ValueError):
            rtx.cosine_directions(bad)
    # a mean of cosines: the directions' z average to 2/3 as k grows (cosine-weighted hemisphere)
    assert abs(float(rtx.cosine_directions(64)[:, 2].mean()) - 2.0 / 3.0) < 0.02


def test_cli_occlusion_arguments(capsys):
    a = cli.parse(["--infile", "s.json", "--occlusion", "o.npz"])
    assert (a.occlusion, a.ao_samples, a.ao_radius, a.outfile) == ("o.npz", None, None, "out.png")
    a = cli.parse(["--infile", "s.json", "--occlusion", "o.npz", "--ao-samples", "8", "--ao-radius", "2.5"])
    assert (a.ao_samples, a.ao_radius) == (8, 2.5)
    a = cli.parse(["--infile", "s.json", "--occlusion", "o.npz", "--aovs", "a.npz", "--subimage", "1", "--tasks", "2"])
    assert (a.occlusion, a.aovs, a.subimage, a.tasks) == ("o.npz", "a.npz", 1, 2)
    a = cli.parse(["--infile", "s.json"])
    assert a.occlusion is None and a.ao_samples is None and a.ao_radius is None   # the ordinary render is unchanged
    for bad, word in ((["--occlusion", "o.npz", "--distributed"], "--distributed"),
                      (["--occlusion", "o.npz", "--frames", "2"], "--frames"),
                      (["--occlusion", "o.npz", "--panorama", "8", "4"], "--panorama"),
                      (["--occlusion", "o.npz", "--ao-samples", "0"], "--ao-samples"),
                      (["--occlusion", "o.npz", "--ao-samples", "65"], "--ao-samples"),
                      (["--occlusion", "o.npz", "--ao-radius", "0"], "--ao-radius"),
                      (["--occlusion", "o.npz", "--ao-radius", "nan"], "--ao-radius"),
                      (["--ao-samples", "4"], "--occlusion"),
                      (["--ao-radius", "1.0"], "--occlusion")):
        with pytest.raises(SystemExit):
            cli.parse(["--infile", "s.json"] + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_writes_the_buffers(tmp_path, monkeypatch):
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(6, 4))
    seen = []

    def fake(buffers, **kw):
        seen.append((tuple(buffers), kw))
        return dict(lights=torch.full((4, 6), -2 ** 31 + 5, dtype=torch.int32),   # bit 31 and bits 0, 2
                    ao=torch.full((4, 6), 0.25, dtype=torch.float32))
    monkeypatch.setattr(sc, "render_occlusion", fake)
    path = str(tmp_path / "occ")                                   # (the name is kept as given)
    args = cli.parse(["--infile", "s.json", "--occlusion", path])
    assert cli.write_occlusion(sc, args) == path
    with np.load(path) as z:
        assert sorted(z.files) == ["ao", "lights"]
        assert z["lights"].dtype == np.uint32 and (z["lights"] == 0x80000005).all() and z["lights"].shape == (4, 6)
        assert z["ao"].dtype == np.float32 and (z["ao"] == 0.25).all()
    args = cli.parse(["--infile", "s.json", "--occlusion", str(tmp_path / "o.npz"), "--subimage", "1", "--tasks", "3",
                      "--ao-samples", "4", "--ao-radius", "1.5"])
    cli.write_occlusion(sc, args)
    assert seen == [(("lights", "ao"), {}), (("lights", "ao"), dict(subimage=1, tasks=3, ao_samples=4, ao_radius=1.5))]


def test_the_numpy_frame_is_orthonormal():
    rng = np.random.RandomState(5)
    n = rng.normal(size=(2000, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    special = [[0, 0, 1], [0, 0, -1], [1, 0, 0.0], [1, 0, -0.0], [0, -1, 0.0], [0.6, 0.8, -0.0], [0, 1e-4, -1],
               [1e-4, 0, 1], [0, 3, 4], [0.2, -0.1, 0.05], [-7, 2, -3], [0, 0, 1e-3], [0, 0, -250.0]]  # (non-unit too)
    n = np.concatenate([np.asarray(special, np.float64), n]).astype(f32)
    T, U, nh = occref.frame(n)
    assert T.dtype == f32 and U.dtype == f32 and nh.dtype == f32
    T, U, nh = (a.astype(np.float64) for a in (T, U, nh))
    dot = lambda a, b: (a * b).sum(axis=1)  # noqa: E731
    for a, b, want in ((T, T, 1), (U, U, 1), (nh, nh, 1), (T, U, 0), (T, nh, 0), (U, nh, 0)):
        assert np.abs(dot(a, b) - want).max() < 5e-7
    assert np.abs(np.cross(T, U) - nh).max() < 5e-7  # right-handed: T x U = n^
    # the poles and the sign of a zero z
    T, U, nh = occref.frame(np.asarray([[0, 0, 1], [0, 0, -1], [1, 0, 0.0], [1, 0, -0.0]], f32))
    assert np.array_equal(T[0], [1, 0, 0]) and np.array_equal(U[0], [0, 1, 0])
    assert np.array_equal(T[1], [1, 0, 0]) and np.array_equal(U[1], [0, -1, 0])
    assert np.array_equal(T[2], [0, 0, -1]) and np.array_equal(T[3], [0, 0, 1])
    # local (0, 0, 1) is the unit normal itself, whatever the frame
    d = occref.ao_rays(n, np.asarray([[0, 0, 1], [1, 0, 0], [0, 1, 0]], f32))
    assert d.shape == (len(n), 3, 3) and d.dtype == f32
    assert np.array_equal(d[:, 0], occref.frame(n)[2])
