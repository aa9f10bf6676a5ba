"""Shading caller-built rays without a GPU: the C entry point's export and argument checks,
the reference camera's rays (Scene.camera_rays) against the restatement of scene.py:54-65 in
tests/test_gpu_aov.py, the panorama camera's geometry, what Scene.cast_rays and
Scene.cast_rays_device refuse before any upload, and the CLI's arguments."""
import math

import numpy as np
import pytest
import torch

import rtx
from common import product_scene
from rtx import _native as N
from rtx import main as cli
from test_gpu_aov import first_sample_rays

f32 = np.float32


def test_entry_point_is_exported_and_the_abi_is_unchanged():
    lib = N.load()
    assert lib.rtx_abi_version() == 6 and N.ABI_VERSION == 6
    assert "rtx_cast_rays" in N.EXPORTS and hasattr(lib, "rtx_cast_rays")
    assert len(lib.rtx_cast_rays.argtypes) == 10
    assert N.RTX_CAST_MAX_TIMES == 64
    assert "panorama_rays" in rtx.__all__


def test_entry_point_refuses_a_null_scene_without_gpu():
    lib = N.load()
    t = (N.C.c_double * 1)(0.0)
    assert lib.rtx_cast_rays(None, 0, None, None, t, 1, 1, None, None, None) == N.RTX_ERR_INVALID
    assert b"rtx_cast_rays: null scene" in lib.rtx_last_error()
    assert lib.rtx_cast_rays(None, 4, 16, 16, t, 1, 1, 16, None, None) == N.RTX_ERR_INVALID
    assert b"rtx_cast_rays: null scene" in lib.rtx_last_error()


def _image(a):
    """[W][H from the bottom][...] (first_sample_rays) as [H from the top][W][...]."""
    return np.swapaxes(a, 0, 1)[::-1]


@pytest.mark.parametrize("name,res,edits,kw", [
    ("TwoSpheresPlane", (11, 7), {"AA": {"jitter": False, "samples": 3}}, {}),
    ("TwoSpheresPlane", (11, 7), {"AA": {"jitter": False, "samples": 3}}, dict(subimage=1, tasks=3)),
    ("DepthOfField", (8, 6), {"AA": {"jitter": False, "samples": 2}}, {}),
])
def test_camera_rays_first_sample_ordering_and_group(name, res, edits, kw):
    sc = product_scene(name, res, **edits)
    o, d, group = sc.camera_rays(**kw)
    t = sc.camera_tables(**kw)
    H, W, nd, na = sc.vc.height, t["ncols"], sc.vc.dof_samples, sc.samples
    assert group == nd * na and (name != "DepthOfField" or nd > 1)
    assert o.dtype == f32 and d.dtype == f32 and o.shape == d.shape == (H * W * group, 3)
    o, d = o.reshape(H, W, nd, na, 3), d.reshape(H, W, nd, na, 3)
    fo, fd = first_sample_rays(sc, **kw)
    assert np.array_equal(o[:, :, 0, 0], _image(fo)) and np.array_equal(d[:, :, 0, 0], _image(fd))
    # every (kd, ka): the origin is aa[kd][ka] at every pixel, the direction depends on kd only
    assert np.array_equal(o, np.broadcast_to(t["aa"].astype(f32).reshape(nd, na, 3), o.shape))
    assert np.array_equal(d, np.broadcast_to(d[:, :, :, :1], d.shape))
    if nd > 1:  # scene.py:58: the sample's direction leaves its own DOF origin toward the pixel's focal point
        from rtx import f32 as F
        vc, r, c, kd = sc.vc, 1, W - 2, nd - 1
        x, y = t["xs"][c], t["ys"][H - 1 - r]
        bdir = F.normalize((x * np.asarray(vc.u, f32) + y * np.asarray(vc.v, f32)) - np.asarray(vc.w, f32) * f32(vc.d))
        focal = np.asarray(vc.position, f32) + bdir * f32(vc.focal_length)
        assert np.array_equal(d[r, c, kd, 0], F.normalize(focal - t["dof"][kd].astype(f32)))
        assert not np.array_equal(d[:, :, 0], d[:, :, kd])
    assert len({o[0, 0, kd, ka].tobytes() for kd in range(nd) for ka in range(na)}) == group


def test_camera_rays_replayed_jitter_and_philox():
    sc = product_scene("DepthOfField", (8, 6), AA={"jitter": True, "samples": 2})
    assert sc.jitter
    with pytest.raises(ValueError, match="Philox"):
        sc.camera_rays()
    nd, na = sc.vc.dof_samples, sc.samples
    noise = np.random.RandomState(5).rand(8 * 6 * nd * na * 3)
    sc.jitter_noise = noise[:-1]
    with pytest.raises(ValueError, match="too short"):
        sc.camera_rays()
    sc.jitter_noise = noise
    o, d, group = sc.camera_rays()
    assert group == nd * na
    o = o.reshape(6, 8, nd, na, 3)
    fo, fd = first_sample_rays(sc, noise=noise)
    assert np.array_equal(o[:, :, 0, 0], _image(fo))
    assert np.array_equal(d.reshape(6, 8, nd, na, 3)[:, :, 0, 0], _image(fd))
    # scene.py:63-65 for another sample: column 5, reference row 1, DOF origin 2, AA origin 1
    t = sc.camera_tables()
    nz = noise.reshape(8, 6, nd, na, 3)[5, 1, 2, 1].astype(f32)
    inv = f32(1.0) / np.sqrt((nz[0] * nz[0] + nz[1] * nz[1]) + nz[2] * nz[2])
    want = t["aa"][2, 1].astype(f32) + (nz * inv) * f32(t["jscale"])
    assert np.array_equal(o[6 - 1 - 1, 5, 2, 1], want)
    assert sc._native is None


@pytest.mark.parametrize("name", ["TwoSpheresPlane", "MirrorRefraction", "DepthOfField", "NovelScene2"])
def test_panorama_rays_geometry(name):
    sc = rtx.load_bundled_scene(name, resolution=(8, 6))
    W, H = 16, 8
    o, d = rtx.panorama_rays(sc.vc, W, H)
    assert o.dtype == f32 and d.dtype == f32 and o.shape == d.shape == (W * H, 3)
    assert np.array_equal(o, np.broadcast_to(np.asarray(sc.vc.position, f32), o.shape))
    d = d.astype(np.float64)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 2.0 ** -23
    u, v, w = (np.asarray(x, np.float64) for x in (sc.vc.u, sc.vc.v, sc.vc.w))
    d = d.reshape(H, W, 3)
    # the four pixels round the image centre straddle the camera's view direction -w symmetrically
    mid = d[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].sum(axis=(0, 1))
    assert np.abs(mid / np.linalg.norm(mid) + w).max() <= 1e-6
    # the two centre columns of a middle row lie at phi = -+ pi / W about -w, left (-u) then right
    for r in (H // 2 - 1, H // 2):
        a, b = d[r, W // 2 - 1], d[r, W // 2]
        assert abs(a @ u + b @ u) <= 1e-6 and a @ u < 0 < b @ u
        assert abs(math.atan2(b @ u, -(b @ w)) - math.pi / W) <= 1e-6
    # the top row points along +v (theta = pi / (2 H) off it), the bottom row along -v
    assert np.abs(d[0] @ v - math.cos(math.pi / (2 * H))).max() <= 1e-6
    assert np.abs(d[H - 1] @ v + math.cos(math.pi / (2 * H))).max() <= 1e-6
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            rtx.panorama_rays(sc.vc, *bad)


def test_cast_rays_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(8, 6))
    o = np.zeros((6, 3), f32)
    d = np.ones((6, 3), f32)
    bad = (
        dict(origins=np.zeros((6, 2), f32)),                 # not [n, 3]
        dict(origins=np.zeros(18, f32)),                     # not two-dimensional
        dict(directions=np.ones((5, 3), f32)),               # another number of rays
        dict(group=0), dict(group=-2), dict(group=4),        # 4 does not divide 6
        dict(group=1.5), dict(group=True),
        dict(times=[]), dict(times=[0.0] * 65), dict(times=[[0.0, 1.0]]),
        dict(times=float("nan")), dict(times=[0.0, float("inf")]), dict(times=1e300), dict(times="soon"),
    )
    for kw in bad:
        args = dict(origins=o, directions=d, times=0.0, group=1)
        args.update(kw)
        with pytest.raises(ValueError):
            sc.cast_rays(**args)
    assert sc._native is None  # nothing was uploaded


def test_cast_rays_device_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(8, 6))
    o, d = torch.zeros((3, 6)), torch.ones((3, 6))
    bad = (
        dict(o=np.zeros((3, 6), f32)),                                  # not a tensor
        dict(o=torch.zeros((3, 6), dtype=torch.float64)),               # not float32
        dict(d=torch.zeros((3, 6), dtype=torch.float16)),
        dict(o=torch.zeros((6, 3))),                                    # not [3, n]
        dict(o=torch.zeros(18)),
        dict(o=torch.zeros((3, 12))[:, ::2]),                           # not contiguous
        dict(d=torch.ones((3, 5))),                                     # another number of rays
        dict(group=4), dict(group=0), dict(times=[]), dict(times=[0.0] * 65), dict(times=float("inf")),
        dict(out=torch.zeros((6, 3), dtype=torch.float64)),             # not float32
        dict(out=torch.zeros((3, 3))),                                  # not [n / group, 3]
        dict(out=torch.zeros((3, 3)), group=3),
        dict(out=np.zeros((6, 3), f32)),
        dict(counters=torch.zeros(4, dtype=torch.int64)),               # too few entries
        dict(counters=torch.zeros(16, dtype=torch.int32)),              # not int64
        {},                                                             # rays that are not on a GPU
    )
    for kw in bad:
        args = dict(o=o, d=d, times=0.0, group=1)
        args.update(kw)
        with pytest.raises(ValueError):
            sc.cast_rays_device(**args)
    with pytest.raises(ValueError, match="CUDA"):
        sc.cast_rays_device(o, d)
    assert sc._native is None  # nothing was uploaded


def test_cli_panorama_arguments(capsys):
    a = cli.parse(["--infile", "s.json", "--outfile", "p.png", "--panorama", "64", "32"])
    assert (a.panorama, a.outfile) == ([64, 32], "p.png")
    assert cli.parse(["--infile", "s.json"]).panorama is None      # the ordinary render is unchanged
    for bad, word in ((["--panorama", "64", "32", "--distributed"], "--panorama"),
                      (["--panorama", "64", "32", "--frames", "2"], "--panorama"),
                      (["--panorama", "64", "32", "--aovs", "o.npz"], "--panorama"),
                      (["--panorama", "64", "32", "--subimage", "0", "--tasks", "2"], "--panorama"),
                      (["--panorama", "0", "32"], "--panorama"),
                      (["--panorama", "64"], "--panorama")):
        with pytest.raises(SystemExit):
            cli.parse(["--infile", "s.json"] + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_panorama_shades_the_panorama_rays(monkeypatch):
    """render_panorama hands panorama_rays, as [3, n] tensors, and the camera's motion times to
    cast_rays_device (the device calls are replaced: no GPU here)."""
    from rtx import scene as S
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    seen = {}

    def fake_cast(o, d, times=0.0, group=1):
        seen.update(o=o, d=d, times=times, group=group)
        return torch.full((o.shape[1], 3), 0.5)

    monkeypatch.setattr(sc, "cast_rays_device", fake_cast)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    monkeypatch.setattr(S, "fb_to_rgb8", lambda fb: (fb * 255.0).to(torch.uint8))
    img = cli.render_panorama(sc, 6, 4)
    assert img.shape == (4, 6, 3) and img.dtype == np.uint8 and (img == 127).all()
    po, pd = rtx.panorama_rays(sc.vc, 6, 4)
    assert np.array_equal(seen["o"].numpy(), po.T) and np.array_equal(seen["d"].numpy(), pd.T)
    assert seen["times"] == [float(t) for t in sc.vc.motion_times] and len(seen["times"]) > 1 and seen["group"] == 1
