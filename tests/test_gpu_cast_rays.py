"""Shading caller-built rays (Scene.cast_rays, rtx_cast_rays) on the GPU, bit for bit.

Two yardsticks, neither of them this kernel: the reference's own function for one ray --
oracle/pyloop.py's PyLoopScene.cast_ray with current_time set (tests/test_pyloop.py holds it
bit-identical to the C oracle) -- and the product's render: the reference camera's sample rays
(Scene.camera_rays) shaded by cast_rays_device must give render_device's framebuffer. Every
comparison is np.array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from rtx import main as cli
from common import OPTS, product_scene_dict
import castref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


def hier_scene(seed, mesh):
    from scenegen import random_hier_scene
    return random_hier_scene(seed, res=(16, 12), mesh=mesh)


# name -> (scene description, probe rays, motion times)
CASES = {
    "TwoSpheresPlane": (lambda: R.bundle("TwoSpheresPlane"), 1500, (0.0,)),
    "MirrorRefraction": (lambda: R.bundle("MirrorRefraction"), 1500, (0.0,)),
    "DepthOfField": (lambda: R.bundle("DepthOfField"), 1500, (0.0,)),
    "MotionBlur": (lambda: R.bundle("MotionBlur"), 900, (0.0, 0.5, 1.0)),
    "TorusMesh flat": (lambda: R.bundle("TorusMesh", flat_shaded=True), 400, (0.0,)),
    "TorusMesh smooth": (lambda: R.bundle("TorusMesh", flat_shaded=False), 400, (0.0,)),
    "NovelScene1": (lambda: R.bundle("NovelScene1"), 300, (0.0,)),
    "NovelScene2": (lambda: R.bundle("NovelScene2"), 300, (0.0, 0.7)),
    "hierarchies 1": (lambda: hier_scene(1, False), 300, (0.0,)),
    "hierarchies 0 with a mesh": (lambda: hier_scene(0, True), 300, (0.0,)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(description, origins, directions, times, PyLoop colours [n][T][3], levels [n][T]): computed
    once per session, shared by the tests, never written to."""
    make, n, times = CASES[name]
    d = make()
    o, dd = R.probe_rays(d, n)
    rgb, levels = R.Reference(d).cast(o, dd, times)
    for a in (o, dd, rgb, levels):
        a.setflags(write=False)
    return d, o, dd, times, rgb, levels


def per_time(sc, o, dd, times):
    """cast_rays one time after the other, group 1: colours [n][T][3]."""
    return np.stack([sc.cast_rays(o, dd, t) for t in times], axis=1)


# ------------------------------------------------------------------ 1. arbitrary rays vs the reference's function
@pytest.mark.parametrize("name", list(CASES))
def test_arbitrary_rays_equal_the_reference_cast_ray(name):
    d, o, dd, times, want, levels = case(name)
    sc = product_scene_dict(d)
    got = per_time(sc, o, dd, times)      # before any camera upload
    assert sc._cam_key is None
    assert got.dtype == f32 and got.shape == want.shape
    # non-vacuity: lit results, and the reflect / refract chain where the scene has one
    assert want.reshape(-1, 3).any(axis=1).mean() >= 0.40, name
    if name == "MirrorRefraction":
        assert (levels >= 2).mean() >= 0.30 and (levels == 10).sum() >= 50
    if name == "NovelScene1":
        assert (levels >= 2).mean() >= 0.30
    unit = np.abs(np.sqrt((dd.astype(np.float64) ** 2).sum(axis=1)) - 1.0) < 1e-6
    assert 0.6 < unit.mean() < 0.9        # directions of other lengths are shaded as given
    assert np.array_equal(got, want), (name, float((got != want).any(axis=2).mean()))
    # every ray at every time in one call: the mean of its times, added in order
    if len(times) > 1:
        assert np.array_equal(sc.cast_rays(o, dd, times), R.ordered_mean(want, 1))


# ------------------------------------------------------------------ 2. the camera's rays vs the render
def _motion(n):
    return {"final": 1, "samples": n - 1, "time": 1.0}


CAMERA = [
    ("TwoSpheresPlane", (50, 37), dict(AA={"jitter": False, "samples": 1}), {}, 1, 1),
    ("MirrorRefraction", (64, 36), {}, {}, 1, 1),
    ("TorusMesh", (48, 48), {}, {}, 1, 1),
    ("TwoSpheresPlane", (50, 37), {}, {}, 3, 1),
    ("DepthOfField", (24, 18), dict(AA={"jitter": False, "samples": 2},
                                    DOF={"aperture": 0.2, "focal_length": 3.0, "samples": 7}), {}, 14, 1),
    ("DepthOfField", (24, 18), dict(AA={"jitter": True, "samples": 2},
                                    DOF={"aperture": 0.2, "focal_length": 3.0, "samples": 7}), {}, 14, 1),
    ("MotionBlur", (30, 26), {}, {}, 1, 17),
    ("NovelScene2", (12, 6), dict(AA={"jitter": False, "samples": 2},
                                  DOF={"aperture": 0.1, "focal_length": 10.0, "samples": 3}, motion=_motion(4)), {}, 6, 4),
    ("TwoSpheresPlane", (50, 37), {}, dict(subimage=1, tasks=3), 3, 1),
]


@pytest.mark.parametrize("name,res,edits,strip,group,ntimes", CAMERA,
                         ids=["%s-%d" % (c[0], i) for i, c in enumerate(CAMERA)])
def test_camera_rays_reproduce_the_render(name, res, edits, strip, group, ntimes, monkeypatch):
    if name == "NovelScene2":  # the generic passes: this camera's CSG-specialized ones take 20 s to compile
        monkeypatch.setattr(OPTS, "jit", "0")
    sc = product_scene_dict(R.bundle(name, res, **edits))
    if sc.jitter:
        sc.jitter_noise = np.random.RandomState(3).rand(res[0] * res[1] * group * 3)
    assert len(sc.vc.motion_times) == ntimes
    cnt_r = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    cnt_c = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    fb = sc.render_device(counters=cnt_r, **strip)
    o, d, g = sc.camera_rays(device=True, **strip)
    assert g == group and o.shape == (3, fb.shape[0] * fb.shape[1] * g)
    got = sc.cast_rays_device(o, d, sc.vc.motion_times, g, counters=cnt_c)
    assert got.shape == (fb.shape[0] * fb.shape[1], 3)
    torch.cuda.synchronize()
    assert fb.cpu().numpy().any()
    assert np.array_equal(got.view(fb.shape).cpu().numpy(), fb.cpu().numpy())
    # casts per level, shadow rays and shade points (not the triangle tests: the bins change them)
    keep = list(range(10)) + [N.RTX_CNT_SHADOW, N.RTX_CNT_SHADE]
    cr, cc = cnt_r.cpu().numpy(), cnt_c.cpu().numpy()
    assert cr[0] == fb.shape[0] * fb.shape[1] * g * ntimes
    assert np.array_equal(cc[keep], cr[keep]), (cc, cr)


# ------------------------------------------------------------------ 3. shapes where the mapping can break
def _tiled(o, dd, n):
    idx = np.arange(n) % len(o)
    return np.ascontiguousarray(o[idx]), np.ascontiguousarray(dd[idx])


# MirrorRefraction runs the flat kernel (256-thread blocks, LDS frames), NovelScene2 the
# hierarchy kernel (64-thread blocks); both on section 1's rays
@pytest.mark.parametrize("name", ["MirrorRefraction", "NovelScene2"])
def test_sample_counts_outputs_and_ragged_blocks(name):
    d, o, dd, _, _, _ = case(name)
    sc = product_scene_dict(d)
    times17 = [k / 16.0 for k in range(17)]
    single = {}  # time -> colours of the base rays, group 1

    def at(t):
        if t not in single:
            single[t] = sc.cast_rays(o, dd, t)
        return single[t]

    # S = group * T: 1; 3 and 14 (several outputs per block, S no divisor of 64 or 256); 64 and 256
    # (exactly one block of the hierarchy / flat kernel); 96 (rounds on the 64-thread block); 680
    # (rounds on both); with one output, with a ragged last block, with several blocks
    shapes = [(1, 1, 1), (1, 1, 65), (3, 1, 100), (1, 3, 100), (7, 2, 1), (7, 2, 41), (64, 1, 3), (256, 1, 2),
              (32, 3, 1), (32, 3, 3), (40, 17, 1), (40, 17, 2)]
    for G, T, nout in shapes:
        times = times17[:T] if T < 17 else times17
        n = G * nout
        idx = np.arange(n) % len(o)
        samples = np.stack([at(t)[idx] for t in times], axis=1)            # [n][T][3]
        want = R.ordered_mean(samples, G)
        oo, do = _tiled(o, dd, n)
        got = sc.cast_rays(oo, do, times, G)
        assert got.shape == (nout, 3) and got.dtype == f32
        assert want.any() and np.array_equal(got, want), (name, G, T, nout)
    # outputs prefilled with NaN, an `out` tensor and counters, asynchronously
    G, T, nout = 7, 2, 41
    n = G * nout
    oo, do = (torch.as_tensor(np.ascontiguousarray(a.T)).cuda() for a in _tiled(o, dd, n))
    out = torch.full((nout + 1, 3), float("nan"), device="cuda")
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    res = sc.cast_rays_device(oo, do, times17[:T], G, out=out[:nout], counters=cnt)
    assert res.data_ptr() == out.data_ptr()
    sc.cast_rays_device(oo, do, times17[:T], G, out=out[:nout], counters=cnt)  # counters accumulate
    torch.cuda.synchronize()
    idx = np.arange(n) % len(o)
    want = R.ordered_mean(np.stack([at(t)[idx] for t in times17[:T]], axis=1), G)
    assert np.array_equal(out[:nout].cpu().numpy(), want)
    assert torch.isnan(out[nout]).all()                                   # nothing past the last output
    assert int(cnt[0]) == 2 * n * T and int(cnt[N.RTX_CNT_SHADE]) > 0
    # no rays: no launch, an empty result
    empty = sc.cast_rays(np.zeros((0, 3), f32), np.zeros((0, 3), f32), [0.0, 1.0], 4)
    assert empty.shape == (0, 3) and empty.dtype == f32


def test_two_calls_with_different_times_on_one_stream():
    """A hierarchy scene's boxes are uploaded per call, in stream order: the second call's boxes
    must not reach the first call's kernel."""
    d, o, dd, times, want, _ = case("NovelScene2")
    sc = product_scene_dict(d)
    od, ddv = (torch.as_tensor(np.ascontiguousarray(a.T)).cuda() for a in (o, dd))
    a = sc.cast_rays_device(od, ddv, times[0])
    b = sc.cast_rays_device(od, ddv, times[1])
    c = sc.cast_rays_device(od, ddv, times[0])
    torch.cuda.synchronize()
    assert not np.array_equal(want[:, 0], want[:, 1])                     # the bike moves
    assert np.array_equal(a.cpu().numpy(), want[:, 0])
    assert np.array_equal(b.cpu().numpy(), want[:, 1])
    assert np.array_equal(c.cpu().numpy(), want[:, 0])


# ------------------------------------------------------------------ 4. not camera rays
def test_rays_leaving_surfaces_ignore_the_cameras_tables():
    """DepthOfField's camera carries the planes' self tests, the directional shadow grids and
    their self boxes (proved for its own rays). Rays that start on the planes' and boxes'
    surfaces and leave at grazing angles must be shaded without them: as the reference does."""
    d = R.bundle("DepthOfField", (24, 18), AA={"jitter": False, "samples": 1},
                 DOF={"aperture": 0.2, "focal_length": 3.0, "samples": 2})
    sc = product_scene_dict(d)
    fb = sc.render_device()
    assert sc._cam_key is not None
    # surface points: where rays from the camera and from about the scene meet planes and boxes
    po, pd = R.probe_rays(d, 6000, seed=11)
    hit = sc.intersect(po, pd)
    kinds = np.array([g["type"] for g in d["objects"]])
    on = (hit["obj"] >= 0) & np.isin(kinds[np.maximum(hit["obj"], 0)], ("plane", "box"))
    on &= np.abs(hit["position"]).max(axis=1) < 30.0
    assert on.sum() >= 600
    p, nrm = hit["position"][on][:600], hit["normal"][on][:600]
    assert {"plane", "box"} <= set(kinds[hit["obj"][on][:600]])
    rs = np.random.RandomState(13)
    centres = np.asarray([g["position"] for g in d["objects"] if g["type"] != "plane"], np.float64)
    toward = centres[rs.randint(len(centres), size=600)] + rs.uniform(-1, 1, (600, 3)) - p
    tangent = toward - nrm * (toward * nrm).sum(axis=1, keepdims=True)
    tangent /= np.linalg.norm(tangent, axis=1, keepdims=True)
    lift = rs.uniform(0.01, 0.2, (600, 1))                                # 0.6 to 11 degrees off the surface
    o = np.ascontiguousarray(p, f32)
    dd = np.ascontiguousarray(tangent + nrm * lift, f32)
    want, _ = R.Reference(d).cast(o, dd, (0.0,))
    assert want[:, 0].any(axis=1).mean() >= 0.25                          # lit surfaces at the far end
    assert np.array_equal(sc.cast_rays(o, dd), want[:, 0])
    # another camera's tables change nothing either
    other = product_scene_dict(R.bundle("DepthOfField", (20, 30), camera=dict(d["camera"], position=[3.0, 2.5, 2.0]),
                                        AA={"jitter": False, "samples": 1},
                                        DOF={"aperture": 0.2, "focal_length": 3.0, "samples": 2}))
    key = sc._cam_key
    sc.vc = other.vc
    fb2 = sc.render_device()
    assert sc._cam_key != key and fb2.shape != fb.shape
    assert np.array_equal(sc.cast_rays(o, dd), want[:, 0])


# ------------------------------------------------------------------ 5. panorama
def test_panorama_equals_the_reference_per_pixel():
    d = R.bundle("MirrorRefraction")
    sc = product_scene_dict(d)
    o, dd = rtx.panorama_rays(sc.vc, 16, 8)
    want, levels = R.Reference(d).cast(o, dd, (0.0,))
    got = sc.cast_rays(o, dd)
    assert want.any(axis=2).mean() >= 0.40 and (levels >= 2).any()
    assert np.array_equal(got, want[:, 0])
    # the CLI's image: main.py:33's bytes of those colours
    img = cli.render_panorama(sc, 16, 8)
    assert img.shape == (8, 16, 3) and img.dtype == np.uint8
    assert np.array_equal(img, (want[:, 0].astype(np.float64) * 255.0).astype(np.uint8).reshape(8, 16, 3))


# ------------------------------------------------------------------ 6. C-level argument errors
@pytest.mark.parametrize("name", ["TwoSpheresPlane", "NovelScene2"])
def test_entry_point_argument_errors_launch_nothing(name):
    d, o, dd, _, _, _ = case(name)
    sc = product_scene_dict(d)
    h = sc.native().h
    lib = N.load()
    n = 12
    od, ddv = (torch.as_tensor(np.ascontiguousarray(a[:n].T)).cuda() for a in (o, dd))
    out = torch.full((n, 3), float("nan"), device="cuda")
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    vp = C.c_void_p
    ro, rd, rgb, cn = vp(od.data_ptr()), vp(ddv.data_ptr()), vp(out.data_ptr()), vp(cnt.data_ptr())

    def times(*t):
        return (C.c_double * max(len(t), 1))(*t)

    t0 = times(0.0)
    big = 1 << 30
    bad = [
        (h, -1, ro, rd, t0, 1, 1, rgb, cn),                               # n < 0
        (h, n, None, rd, t0, 1, 1, rgb, cn),                              # null rays
        (h, n, ro, None, t0, 1, 1, rgb, cn),
        (h, n, ro, rd, t0, 1, 1, None, cn),                               # null output
        (h, n, ro, rd, t0, 1, 0, rgb, cn),                                # group < 1
        (h, n, ro, rd, t0, 1, -3, rgb, cn),
        (h, n, ro, rd, t0, 1, 5, rgb, cn),                                # group does not divide n
        (h, n, ro, rd, t0, 0, 1, rgb, cn),                                # n_times < 1
        (h, n, ro, rd, times(*([0.0] * 65)), 65, 1, rgb, cn),             # n_times above the cap
        (h, n, ro, rd, None, 1, 1, rgb, cn),                              # null times
        (h, n, ro, rd, times(0.0, float("nan")), 2, 1, rgb, cn),          # non-finite times
        (h, n, ro, rd, times(float("inf")), 1, 1, rgb, cn),
        (h, n, ro, rd, times(1e300), 1, 1, rgb, cn),                      # (not finite as fp32)
        (h, big, ro, rd, times(0.0, 1.0), 2, big, rgb, cn),               # group * n_times >= 2^31
        (h, 1 << 40, ro, rd, t0, 1, 1, rgb, cn),                          # more blocks than a grid holds
        (None, n, ro, rd, t0, 1, 1, rgb, cn),                             # null scene
    ]
    for args in bad:
        assert lib.rtx_cast_rays(*args, None) == N.RTX_ERR_INVALID, args[1:]
        assert b"rtx_cast_rays" in lib.rtx_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and int(cnt.sum()) == 0                 # nothing ran
    assert lib.rtx_cast_rays(h, 0, None, None, t0, 1, 1, None, None, None) == N.RTX_OK
    assert lib.rtx_cast_rays(h, n, ro, rd, times(0.0, 0.5), 2, 3, rgb, cn, None) == N.RTX_OK
    torch.cuda.synchronize()
    assert not torch.isnan(out[:n // 3]).any() and torch.isnan(out[n // 3:]).all() and int(cnt[0]) == 2 * n
    assert sc.last_kernel == ""                                           # rtx_last_kernel is left as it is
