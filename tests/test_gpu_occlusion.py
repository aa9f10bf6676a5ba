"""Occlusion buffers (Scene.render_occlusion, rtx_render_occlusion) on the GPU, bit for bit
against the oracle.

The expected values come from two things: the hit points and normals that render_aovs stores
in the SAME camera state (so Philox-jittered cameras work), and OracleScene.shadow for the
rays restated in numpy fp32 (tests/occref.py): a light's shadow ray from p, and the
ambient-occlusion rays in the orthonormal frame of rtx.h. Every comparison is np.array_equal.

Non-vacuity (asserted): on TwoSpheresPlane, TorusMesh and MirrorRefraction at least 5 % of the
hit pixels have a cleared bit of some light and at least 5 % a set one, and with unbounded rays
at least 25 % have 0 < ao < 1. The oracle alone gives, for rtx.cosine_directions(16) as rtx.h
and its docstring define them (fp64 sunflower points rounded once): partial AO 0.37 / 0.61 /
0.92 on the three scenes and 0.48 on MotionBlur; with ao_radius = 1.0 TwoSpheresPlane has 0.15
(its ground is partly open only within one unit of a sphere), so that case asserts that the
bounded rays change the buffer and leave partial pixels, not the 25 %."""
import copy
import os

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from common import OPTS, product_scene_dict
from oracle import oracle as O
import occref

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")
f32 = np.float32
INF = float("inf")


def bundle(name, res, **edits):
    d, _ = O.load_bundle(name)
    d = copy.deepcopy(d)
    d["resolution"] = list(res)
    d.update(edits)
    return d


def host(buffers):
    torch.cuda.synchronize()
    out = {n: t.cpu().numpy() for n, t in buffers.items()}
    if "lights" in out:
        assert out["lights"].dtype == np.int32
        out["lights"] = out["lights"].view(np.uint32)
    return out


def want_for(d, sc, dirs, radius=INF, time=None, base=ASSETS, **camera):
    """(lights, ao, hit) expected for the scene's current camera arguments."""
    aov = host(sc.render_aovs(("position", "normal", "depth"), **camera))
    if time is None:
        time = float(sc.vc.motion_times[0])
    return occref.expected(occref.oracle_scene(d, base), sc.lights, aov, time, dirs, radius) + (aov,)


def run_case(d, what, K=16, radius=INF, base=ASSETS):
    sc = product_scene_dict(d)
    got = host(sc.render_occlusion(ao_samples=K, ao_radius=radius))
    H, W = sc.vc.height, sc.vc.width
    assert got["lights"].shape == (H, W) and got["ao"].shape == (H, W) and got["ao"].dtype == np.float32
    want_l, want_a, hit, aov = want_for(d, sc, rtx.cosine_directions(K), radius, base=base)
    print("%s: hit %.2f, lit per light %s, partial ao %.2f, mean ao %.3f" % (
        what, hit.mean(), [round(float(((want_l[hit] >> i) & 1).mean()), 2) for i in range(len(sc.lights))],
        ((want_a[hit] > 0) & (want_a[hit] < 1)).mean() if hit.any() else 0.0, want_a.mean()))
    assert np.array_equal(got["lights"], want_l), what
    assert np.array_equal(got["ao"], want_a), what
    assert (got["lights"][~hit] == 0).all() and (got["ao"][~hit] == 1.0).all(), what
    return sc, got, hit, aov


def lights_by_occluded(sc, aov, hit, time):
    """The mask from Scene.occluded (rtx_occluded), one call per light."""
    p = aov["position"][hit]
    m = np.zeros(len(p), np.uint32)
    for i, (dr, tm) in enumerate(occref.light_rays(sc.lights, p)):
        free = ~sc.occluded(p, dr, tm, time)
        m |= np.where(free, np.uint32(1 << i), np.uint32(0)).astype(np.uint32)
    out = np.zeros(hit.shape, np.uint32)
    out[hit] = m
    return out


BUNDLED = [("TwoSpheresPlane", (50, 37), INF), ("TwoSpheresPlane", (50, 37), 1.0), ("TorusMesh", (32, 32), INF),
           ("MirrorRefraction", (48, 27), INF), ("MotionBlur", (32, 24), INF), ("DepthOfField", (32, 24), INF)]


@pytest.mark.parametrize("name,res,radius", BUNDLED, ids=["%s-%s" % (n, r) for n, _, r in BUNDLED])
def test_bundled_scenes_match_the_oracle(name, res, radius):
    d = bundle(name, res)
    sc, got, hit, aov = run_case(d, name, 16, radius)
    assert hit.mean() > 0.5
    assert np.array_equal(got["lights"], lights_by_occluded(sc, aov, hit, float(sc.vc.motion_times[0]))), name
    full = np.uint32((1 << len(sc.lights)) - 1)
    li, ao = got["lights"][hit], got["ao"][hit]
    partial = ((ao > 0) & (ao < 1)).mean()
    if name in ("TwoSpheresPlane", "TorusMesh", "MirrorRefraction"):
        assert (li != full).mean() >= 0.05 and (li != 0).mean() >= 0.05, name
        if radius == INF:
            assert partial >= 0.25, (name, partial)
        else:  # bounded rays: fewer of them end on something
            far = host(sc.render_occlusion("ao", ao_samples=16))["ao"]
            assert partial > 0.05 and (got["ao"] >= far).all() and (got["ao"] > far).mean() > 0.05
    if name == "MotionBlur":
        assert partial >= 0.25, (name, partial)


@pytest.mark.parametrize("name", ["NovelScene1", "NovelScene2"])
def test_novel_scenes_match_the_oracle(name):
    """Hierarchies and textures (the X kernels)."""
    sc, got, hit, _ = run_case(bundle(name, (32, 16)), name, K=8)
    assert hit.any() and len(np.unique(got["ao"])) > 2


@pytest.mark.parametrize("seed,mesh", [(0, False), (1, True)])
def test_random_hierarchy_scenes_match_the_oracle(seed, mesh):
    from scenegen import random_hier_scene
    run_case(random_hier_scene(seed, mesh=mesh), "hier %d" % seed, K=8)


@pytest.mark.parametrize("K", [1, 17, 64])
def test_direction_counts(K):
    d = bundle("TwoSpheresPlane", (26, 19))
    _, got, hit, _ = run_case(d, "K = %d" % K, K=K)
    steps = np.unique(got["ao"][hit])
    assert set(steps.tolist()) <= set((np.arange(K + 1, dtype=f32) / f32(K)).tolist())
    assert len(steps) >= 2


def test_row_blocks_and_strips_equal_the_full_pass():
    for d in (bundle("TorusMesh", (50, 37)), bundle("NovelScene1", (50, 37))):
        sc = product_scene_dict(d)
        full = host(sc.render_occlusion(ao_samples=8))
        rows = host(sc.render_occlusion(ao_samples=8, row0=3, nrows=13))   # off the 8-row grid of the bins
        for n in full:
            assert np.array_equal(rows[n], full[n][3:16]), n
        col0, ncols = rtx.strip_columns(50, 1, 3)
        part = host(sc.render_occlusion(ao_samples=8, subimage=1, tasks=3))
        for n in full:
            assert part[n].shape == (37, ncols) and np.array_equal(part[n], full[n][:, col0:col0 + ncols]), n
        want_l, want_a, hit, _ = want_for(d, sc, rtx.cosine_directions(8), row0=3, nrows=13)
        assert np.array_equal(rows["lights"], want_l) and np.array_equal(rows["ao"], want_a) and hit.any()
        empty = sc.render_occlusion(row0=5, nrows=0)
        assert empty["lights"].shape == (0, 50) and empty["ao"].shape == (0, 50)


def test_selection_and_out_tensors():
    sc = product_scene_dict(bundle("TwoSpheresPlane", (50, 37)))
    full = host(sc.render_occlusion())
    ao = torch.full((37, 50), float("nan"), device="cuda")
    li = torch.full((37, 50), -7, dtype=torch.int32, device="cuda")
    # each buffer alone: the other tensor is left as it was
    got = sc.render_occlusion("lights", out=dict(lights=li))
    assert list(got) == ["lights"] and got["lights"] is li
    torch.cuda.synchronize()
    assert np.array_equal(li.cpu().numpy().view(np.uint32), full["lights"]) and bool(torch.isnan(ao).all())
    li.fill_(-7)
    got = sc.render_occlusion(("ao",), out=dict(ao=ao))
    assert list(got) == ["ao"] and got["ao"] is ao
    torch.cuda.synchronize()
    assert np.array_equal(ao.cpu().numpy(), full["ao"]) and bool((li == -7).all())
    # a partial out: the other requested buffer is allocated
    ao.fill_(float("nan"))
    got = sc.render_occlusion(out=dict(ao=ao))
    assert list(got) == ["lights", "ao"] and got["ao"] is ao
    got = host(got)
    assert np.array_equal(got["ao"], full["ao"]) and np.array_equal(got["lights"], full["lights"])
    with pytest.raises(ValueError):
        sc.render_occlusion("ao", out=dict(ao=torch.empty((50, 37), device="cuda").t()))  # not contiguous
    with pytest.raises(ValueError):
        sc.render_occlusion("lights", out=dict(lights=torch.empty((37, 50), dtype=torch.int64, device="cuda")))


def test_caller_directions_and_one_below_the_horizon():
    d = bundle("TwoSpheresPlane", (50, 37))
    sc = product_scene_dict(d)
    rng = np.random.RandomState(3)
    dirs = rng.normal(size=(5, 3))
    dirs[:, 2] = np.abs(dirs[:, 2])
    dirs[1] *= 3.0                      # not unit: used as given
    dirs = dirs.astype(f32)
    got = host(sc.render_occlusion("ao", ao_dirs=dirs, ao_samples=0))["ao"]   # (ao_samples is not read)
    _, want_a, hit, aov = want_for(d, sc, dirs)
    assert np.array_equal(got, want_a) and len(np.unique(got[hit])) > 2
    # one direction pointing below the surface: it ends inside the sphere it starts on, and on
    # nothing under the ground plane (the reference's shadow rays have no back-face rule)
    down = np.asarray([[0.3, 0.1, -1.0]], f32)
    got = host(sc.render_occlusion("ao", ao_dirs=down))["ao"]
    _, want_a, hit, _ = want_for(d, sc, down)
    assert np.array_equal(got, want_a)
    assert (got[hit] == 0.0).any() and (got[hit] == 1.0).any() and set(np.unique(got).tolist()) <= {0.0, 1.0}


def test_sequence_frames():
    d = bundle("MotionBlur", (32, 24))
    windows = rtx.frame_windows(0, 2, 3)
    sc = product_scene_dict(d)
    frames = [host(sc.render_occlusion(ao_samples=8, windows=windows, frame=k)) for k in range(2)]
    for k in range(2):
        want_l, want_a, hit, _ = want_for(d, sc, rtx.cosine_directions(8), time=windows[k][0], windows=windows, frame=k)
        assert np.array_equal(frames[k]["lights"], want_l) and np.array_equal(frames[k]["ao"], want_a), k
    assert not np.array_equal(frames[0]["ao"], frames[1]["ao"])  # the scene moves
    with pytest.raises(ValueError):
        sc.render_occlusion(windows=windows, frame=3)


def _culling_scenes():
    from scenegen import random_hier_scene, random_scene, shadow_scene
    yield "TwoSpheresPlane", bundle("TwoSpheresPlane", (50, 37))
    yield "TorusMesh", bundle("TorusMesh", (32, 32))
    yield "shadow_scene", shadow_scene(0)
    yield "random", random_scene(1, res=(40, 30), mesh=True)
    yield "hier", random_hier_scene(2)


def test_culling_structures_change_nothing(monkeypatch):
    """The lights' tests use the camera's shadow bins, plane self tests, directional shadow
    grids and the light grids, like a render's; the ambient-occlusion rays use none. With all
    of them off the bits are the same."""
    scenes = list(_culling_scenes())
    on = [host(product_scene_dict(d).render_occlusion(ao_samples=8)) for _, d in scenes]
    for opt in ("bins", "shadow_bins", "self_skip", "dsgrid", "lgrid"):
        monkeypatch.setattr(OPTS, opt, "0")   # (read when the camera is uploaded; restored at teardown)
    for (what, d), a in zip(scenes, on):
        b = host(product_scene_dict(d).render_occlusion(ao_samples=8))
        assert np.array_equal(a["lights"], b["lights"]) and np.array_equal(a["ao"], b["ao"]), what
    assert all(a["lights"].any() and (a["ao"] < 1).any() for a in on[:4])


def test_a_render_in_between_changes_nothing(monkeypatch):
    """A render leaves per-scene state behind (the heavy tiles' chunk results, the split
    passes' scratch); the pass reads none of it."""
    monkeypatch.setattr(OPTS, "jit", "0")   # the precompiled render kernels: no compile to wait for
    for d in (bundle("TorusMesh", (32, 32)), bundle("NovelScene2", (32, 16))):
        sc = product_scene_dict(d)
        a = host(sc.render_occlusion(ao_samples=8))
        sc.render()
        b = host(sc.render_occlusion(ao_samples=8))
        assert np.array_equal(a["lights"], b["lights"]) and np.array_equal(a["ao"], b["ao"])


def _ring_of_lights(n, res=(16, 12)):
    """TwoSpheresPlane under n point lights on a ring, every third one under the ground."""
    d = bundle("TwoSpheresPlane", res)
    proto = next(L for L in d["lights"] if L["type"] == "point")
    d["lights"] = []
    for i in range(n):
        a = 2.0 * np.pi * i / 32.0
        y = -3.0 if i % 3 == 1 else 4.0 + 0.1 * i
        d["lights"].append(dict(copy.deepcopy(proto), name="ring%d" % i,
                                position=[round(5.0 * np.cos(a), 3), y, round(5.0 * np.sin(a), 3)]))
    return d


def test_32_lights_fill_the_mask():
    d = _ring_of_lights(32)
    sc, got, hit, aov = run_case(d, "32 lights", K=4)
    li = got["lights"][hit]
    assert ((li >> 31) & 1).any() and not ((li >> 31) & 1).all()       # bit 31 set and cleared
    assert len(np.unique(li)) > 4
    assert np.array_equal(got["lights"], lights_by_occluded(sc, aov, hit, 0.0))
    assert (sc.render_occlusion("lights")["lights"] < 0).any().item()  # int32 on the device: bit 31 is the sign


def test_33_lights_keep_ambient_occlusion_only():
    d = _ring_of_lights(33)
    sc = product_scene_dict(d)
    for names in (("lights", "ao"), "lights"):
        with pytest.raises(ValueError, match="32 lights"):
            sc.render_occlusion(names)
    got = host(sc.render_occlusion("ao", ao_samples=4))["ao"]
    _, want_a, hit, _ = want_for(d, sc, rtx.cosine_directions(4))
    assert np.array_equal(got, want_a) and hit.any()
    # the C call refuses the mask too, and writes nothing
    lib = N.load()
    buf = torch.full((12, 16), -7, dtype=torch.int32, device="cuda")
    ao = torch.full((12, 16), float("nan"), device="cuda")
    dirs = np.ascontiguousarray(rtx.cosine_directions(4))
    rc = lib.rtx_render_occlusion(sc.native().h, 0, 12, 0, buf.data_ptr(), ao.data_ptr(),
                                  dirs.ctypes.data_as(N.C.POINTER(N.C.c_float)), 4, INF, None)
    assert rc == N.RTX_ERR_INVALID and b"32 lights" in lib.rtx_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -7).all()) and bool(torch.isnan(ao).all())


def test_no_lights():
    d = bundle("TwoSpheresPlane", (26, 19), lights=[])
    _, got, hit, _ = run_case(d, "no lights", K=4)
    assert not got["lights"].any() and hit.any() and (got["ao"][hit] < 1).any()


def test_entry_point_argument_errors():
    lib = N.load()
    sc = product_scene_dict(bundle("TwoSpheresPlane", (16, 8)))
    h = sc.native().h
    li = torch.full((8, 16), -7, dtype=torch.int32, device="cuda")
    ao = torch.full((8, 16), float("nan"), device="cuda")
    pl, pa = li.data_ptr(), ao.data_ptr()
    fp = N.C.POINTER(N.C.c_float)
    good = np.ascontiguousarray(rtx.cosine_directions(4))
    nan_dir, inf_dir = good.copy(), good.copy()
    nan_dir[2, 1] = np.nan
    inf_dir[3, 2] = np.inf
    gp = good.ctypes.data_as(fp)

    def untouched():
        torch.cuda.synchronize()
        return bool((li == -7).all()) and bool(torch.isnan(ao).all())

    assert lib.rtx_render_occlusion(h, 0, 8, 0, pl, pa, gp, 4, INF, None) == N.RTX_ERR_STATE
    assert b"rtx_render_occlusion: rtx_camera_set" in lib.rtx_last_error() and untouched()
    sc.render_aovs(("depth",))   # uploads the camera
    kernel = sc.last_kernel
    bad = [(0, 9, 0, pl, pa, gp, 4, INF), (-1, 2, 0, pl, pa, gp, 4, INF), (4, -1, 0, pl, pa, gp, 4, INF),
           (7, 2, 0, pl, pa, gp, 4, INF),                                   # rows outside the image
           (0, 8, 0, None, None, gp, 4, INF),                               # no buffer
           (0, 8, 1, pl, pa, gp, 4, INF), (0, 8, -1, pl, pa, gp, 4, INF),   # frame outside the sequence
           (0, 8, 0, pl, pa, None, 4, INF), (0, 8, 0, None, pa, None, 4, INF),  # no directions
           (0, 8, 0, pl, pa, gp, 0, INF), (0, 8, 0, pl, pa, gp, -1, INF), (0, 8, 0, pl, pa, gp, 65, INF),
           (0, 8, 0, pl, pa, nan_dir.ctypes.data_as(fp), 4, INF), (0, 8, 0, pl, pa, inf_dir.ctypes.data_as(fp), 4, INF),
           (0, 8, 0, pl, pa, gp, 4, 0.0), (0, 8, 0, pl, pa, gp, 4, -1.0), (0, 8, 0, pl, pa, gp, 4, float("nan")),
           (0, 8, 0, pl, pa, gp, 4, -INF)]
    for args in bad:
        assert lib.rtx_render_occlusion(h, *args, None) == N.RTX_ERR_INVALID, args
        assert lib.rtx_last_error().startswith(b"rtx_render_occlusion: "), args
        assert untouched(), args
    assert lib.rtx_render_occlusion(h, 8, 0, 0, pl, pa, gp, 4, INF, None) == N.RTX_OK and untouched()  # no rows
    # without `ao`, its arguments are not looked at
    assert lib.rtx_render_occlusion(h, 0, 8, 0, pl, None, None, -5, float("nan"), None) == N.RTX_OK
    torch.cuda.synchronize()
    assert bool((li != -7).all()) and bool(torch.isnan(ao).all())
    want = host(sc.render_occlusion())
    assert np.array_equal(li.cpu().numpy().view(np.uint32), want["lights"])
    assert lib.rtx_render_occlusion(h, 0, 8, 0, None, pa, gp, 4, 2.5, None) == N.RTX_OK
    assert np.array_equal(host(dict(ao=ao))["ao"], host(sc.render_occlusion("ao", ao_samples=4, ao_radius=2.5))["ao"])
    windows = rtx.frame_windows(0, 1, 2)
    sc.render_occlusion(windows=windows, frame=1)
    assert lib.rtx_render_occlusion(h, 0, 8, 2, pl, pa, gp, 4, INF, None) == N.RTX_ERR_INVALID
    assert b"frame 2" in lib.rtx_last_error()
    assert sc.last_kernel == kernel == ""  # rtx_last_kernel is left as it is
    torch.cuda.synchronize()
