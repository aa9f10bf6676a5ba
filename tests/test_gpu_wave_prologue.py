"""The one-sample scene-specialized kernels' prologue on the MI355X (rtx_kernels.h render_body,
RTX_WAVE_HEAD): the frame parameters come by value from the camera block at the head of
KParams (with rtx_camera_set's copies of dof_o[0] and aa_o[0]), the pixel tables and the tile's
object mask are addressed from Launch's pointers, and the block size is a constant of the
kernel. None of it changes a value: every frame equals the oracle's and the generic kernel's,
bit for bit, in every launch form, and a camera upload refreshes the copies."""
import copy

import numpy as np
import pytest
import torch

import rtx
from common import OPTS, assert_parity, oracle_render, oracle_render_dict, product_scene, product_scene_dict
from rtx import _native as N
from rtx.io import bundled_scene_dict

pytestmark = pytest.mark.gpu

ONE = {"AA": {"jitter": False, "samples": 1}}


def _specialized(sc):
    """The scene with its specialized kernel compiled and picked up."""
    sc.render_device()
    assert sc.jit_wait() == 0
    sc.render_device()
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    return sc


def _generic_frame(make, monkeypatch):
    """(fp32 frame, tallies) of the precompiled generic kernel."""
    monkeypatch.setattr(OPTS, "jit", "0")
    sc = make()
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    fb = sc.render_device(counters=cnt).clone()
    assert sc.last_kernel.startswith("k_render"), sc.last_kernel
    monkeypatch.setattr(OPTS, "jit", "1")
    return fb, cnt.cpu().numpy()


def _rgb8_of(fb):
    """main.py:33's (v * 255).astype(uint8) of an fp32 frame (values in [0, 1])."""
    return (fb.double() * 255.0).to(torch.int32).to(torch.uint8)


def _flat(n_spheres=5, n_lights=2, res=(96, 72)):
    """A checker ground, n_spheres spheres and two boxes on four materials under n_lights
    lights (point and directional in turn), one sample per pixel."""
    rng = np.random.RandomState(4100 + 10 * n_spheres + n_lights)
    r = lambda lo, hi, n=None: np.round(rng.uniform(lo, hi, n), 3).tolist()  # noqa: E731
    mats = [{"name": "m%d" % i, "ID": i, "type": "diffuse", "diffuse": r(0.1, 1, 3), "specular": r(0, 1, 3),
             "hardness": [0, 16, 50, 16][i]} for i in range(4)]
    objs = [{"name": "ground", "type": "plane", "normal": [0.0, 1.0, 0.0], "position": [0.0, -1.0, 0.0],
             "materials": [0, 1]}]
    for k in range(n_spheres):
        rad = float(r(0.2, 0.8))
        pos = r(-3.5, 3.5, 3)
        if k % 2:
            pos[1] = round(-1.0 + rad, 3)  # resting on the ground
        objs.append({"name": "s%d" % k, "type": "sphere", "radius": rad, "position": pos, "materials": [k % 4]})
    for k in range(2):
        sz = r(0.4, 1.4, 3)
        pos = r(-3, 3, 3)
        pos[1] = round(-1.0 + sz[1] / 2, 3)
        objs.append({"name": "b%d" % k, "type": "box", "position": pos, "size": sz, "materials": [2 + k]})
    lights = []
    for i in range(n_lights):
        if i % 2:
            lights.append({"name": "d%d" % i, "type": "directional", "direction": [float(r(-1, 1)), -1.0, float(r(-1, 1))],
                           "colour": r(0.2, 1, 3), "power": float(r(0.2, 0.6))})
        else:
            pos = r(-7, 7, 3)
            pos[1] = abs(pos[1]) + 2.0
            lights.append({"name": "p%d" % i, "type": "point", "position": pos, "colour": r(0.2, 1, 3),
                           "power": float(r(0.3, 0.9))})
    return {"resolution": list(res), "AA": {"jitter": False, "samples": 1}, "ambient": [0.1, 0.1, 0.1],
            "camera": {"position": [1.0, 2.5, 8.0], "lookAt": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "fov": 50.0},
            "materials": mats, "objects": objs, "lights": lights}


@pytest.mark.parametrize("res", [(96, 72), (50, 37)])
def test_two_spheres_plane_launch_forms(res, monkeypatch):
    """Whole frame, a row block off the 8-row grid, two groups, a batch of two frames and uint8
    output, at a frame of whole tiles and one with edge tiles in both directions."""
    W, H = res
    ref = oracle_render("TwoSpheresPlane", res, **ONE)
    sc = _specialized(product_scene("TwoSpheresPlane", res, **ONE))
    assert_parity(sc.render(), ref, "TwoSpheresPlane %s" % (res,))
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    full = sc.render_device(counters=cnt).clone()
    sc.jit_wait()
    assert torch.equal(sc.render_device(), full)  # (the kernel without counters)
    gen, gen_cnt = _generic_frame(lambda: product_scene("TwoSpheresPlane", res, **ONE), monkeypatch)
    assert torch.equal(full, gen)
    assert np.array_equal(cnt.cpu().numpy()[:12], gen_cnt[:12]), (cnt, gen_cnt)
    assert torch.equal(sc.render_device(row0=3, nrows=13), full[3:16])
    rows = torch.as_tensor(rtx.scene.group_rows(H, 2, 1), device="cuda")
    assert torch.equal(sc.render_device(groups=(1, 2)), full[rows])
    out = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda")
    sc.render_frames(out)
    assert torch.equal(out[0], full) and torch.equal(out[1], full)
    u8 = sc.render_device(rgb8=True).clone()
    sc.jit_wait()
    u8 = sc.render_device(rgb8=True)
    assert sc.last_kernel.startswith("rtx_jit_render_") and sc.last_kernel.endswith("_rgb8"), sc.last_kernel
    assert torch.equal(u8, _rgb8_of(full))
    assert torch.equal(sc.render_device(row0=3, nrows=13, rgb8=True), _rgb8_of(full)[3:16])


def test_column_strip():
    """A strip with col0 > 0: its own pixel table and bins."""
    res = (50, 37)
    ref = oracle_render("TwoSpheresPlane", res, subimage=1, tasks=2, **ONE)
    sc = product_scene("TwoSpheresPlane", res, **ONE)
    sc.render(subimage=1, tasks=2)
    assert sc.jit_wait() == 0
    img = sc.render(subimage=1, tasks=2)
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    assert_parity(img, ref, "TwoSpheresPlane strip 1 of 2")


def test_camera_moved_between_renders():
    """A second rtx_camera_set with the eye moved: stale copies of dof_o[0] / aa_o[0] (or of the
    origin terms beside them) would render the first camera's rays."""
    res = (96, 72)
    d = bundled_scene_dict("TwoSpheresPlane", resolution=res)
    d.update(copy.deepcopy(ONE))
    sc = _specialized(product_scene_dict(d))
    first = sc.render_device().clone()
    eye, look, up, fov = [1.5, 3.0, 7.0], [0.0, 0.5, 0.0], [0.0, 1.0, 0.0], 40
    sc.vc.set_camera(eye, look, up, fov)
    moved = sc.render_device().clone()
    sc.jit_wait()
    assert torch.equal(sc.render_device(), moved)
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    assert not torch.equal(moved, first)
    fresh = product_scene_dict(d)
    fresh.vc.set_camera(eye, look, up, fov)
    assert torch.equal(_specialized(fresh).render_device(), moved)
    e = copy.deepcopy(d)
    e["camera"] = {"position": eye, "lookAt": look, "up": up, "fov": fov}
    assert_parity(sc.render(), oracle_render_dict(e), "TwoSpheresPlane, camera moved")


def test_sequence_camera_two_windows():
    """A sequence camera (two windows of motion times) of a scene with a moving sphere."""
    d = _flat(5, 2)
    d["objects"][1]["speed"] = [0.4, 0.0, -0.3]
    times = [0.0, 1.25]
    fb = product_scene_dict(d).render_sequence(times).clone()
    for f, t in enumerate(times):
        e = copy.deepcopy(d)
        e["motion"] = {"time": t, "samples": 0, "final": 1}
        got = np.ascontiguousarray(np.transpose(fb[f].cpu().numpy()[::-1], (1, 0, 2))).astype(np.float64)
        assert_parity(got, oracle_render_dict(e), "moving sphere t=%g" % t)


@pytest.mark.parametrize("n_spheres,n_lights", [(5, 2), (5, 3), (5, 4), (17, 2)])
def test_flat_scenes(n_spheres, n_lights, monkeypatch):
    """A checker plane, spheres and boxes on four materials; three and four lights; 17 spheres
    (past the tile mask's 16 sphere bits)."""
    d = _flat(n_spheres, n_lights)
    ref = oracle_render_dict(d)
    sc = _specialized(product_scene_dict(d))
    assert_parity(sc.render(), ref, "flat %d spheres %d lights" % (n_spheres, n_lights))
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    fb = sc.render_device(counters=cnt).clone()
    sc.jit_wait()
    fb = sc.render_device(counters=cnt.zero_()).clone()
    gen, gen_cnt = _generic_frame(lambda: product_scene_dict(d), monkeypatch)
    assert torch.equal(fb, gen)
    assert np.array_equal(cnt.cpu().numpy()[:12], gen_cnt[:12]), (cnt, gen_cnt)
    assert torch.equal(sc.render_device(row0=3, nrows=13), fb[3:16])


@pytest.mark.parametrize("name,res", [("MirrorRefraction", (64, 36)), ("TorusMesh", (48, 48))])
def test_secondary_rays_and_mesh(name, res, monkeypatch):
    """MirrorRefraction (secondary rays, no shadow table) and TorusMesh (face bins)."""
    ref = oracle_render(name, res, **ONE)
    sc = _specialized(product_scene(name, res, **ONE))
    assert_parity(sc.render(), ref, name)
    fb = sc.render_device().clone()
    gen, _ = _generic_frame(lambda: product_scene(name, res, **ONE), monkeypatch)
    assert torch.equal(fb, gen)
    assert torch.equal(sc.render_device(row0=3, nrows=13), fb[3:16])
    rows = torch.as_tensor(rtx.scene.group_rows(res[1], 2, 1), device="cuda")
    assert torch.equal(sc.render_device(groups=(1, 2)), fb[rows])
