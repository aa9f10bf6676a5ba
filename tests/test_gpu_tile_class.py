"""Tile classes on the MI355X (option tile_class; rtx_api.hip sb_bin, k_shadow_bins; rtx_kernels.h
render_body, RTX_TILE_CLASS): SKY waves store a miss at once and UNSHADOWED waves shade the
plane without a shadow test, only where that is proven for every pixel of the tile -- so a
frame equals the oracle's, the frame with tile_class 0 and the generic kernel's, bit for bit,
fp32 and uint8, in every launch form, and so do the ray tallies."""
import copy

import numpy as np
import pytest
import torch

import rtx
from class_scenes import constructed
from common import OPTS, assert_parity, oracle_render, oracle_render_dict, product_scene, product_scene_dict
from rtx import _native as N
from shadow_scenes import TANGENT_CASES, tangent_scene

pytestmark = pytest.mark.gpu

ONE = {"AA": {"jitter": False, "samples": 1}}
SIZES = [(72, 40), (61, 35)]
MACRO = "'-DRTX_TILE_CLASS=1'"


def _forms(sc, H, jit=True, u8=True):
    """Every launch form of one camera with the scene-specialized kernel (jit) or the generic one:
    whole frame fp32 (twice: with tallies and without) and uint8, a row block off the 8-row grid,
    interleaved groups."""
    sc.render_device()
    assert sc.jit_wait() == 0
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    out = {"fb": sc.render_device(counters=cnt).clone()}
    sc.jit_wait()
    out["fb_plain"] = sc.render_device().clone()
    assert sc.last_kernel.startswith("rtx_jit_render_") == jit, sc.last_kernel
    out["kernel"] = sc.last_kernel
    out["cnt"] = cnt.cpu().numpy()
    out["blk"] = sc.render_device(row0=3, nrows=H - 5).clone()
    out["grp"] = sc.render_device(groups=(1, 2)).clone()
    if u8:
        sc.render_device(rgb8=True)
        sc.jit_wait()
        out["u8"] = sc.render_device(rgb8=True).clone()
        out["u8_blk"] = sc.render_device(row0=3, nrows=H - 5, rgb8=True).clone()
    torch.cuda.synchronize()
    return out


def _same(a, b, what):
    for k in ("fb", "fb_plain", "blk", "grp", "u8", "u8_blk"):
        if k not in a:
            continue
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), "%s: %s differs" % (what, k)
    assert np.array_equal(a["cnt"], b["cnt"]), (what, a["cnt"], b["cnt"])


def _all_ways(make, H, monkeypatch, what, u8=True):
    """The scene's forms with the option as it is by default (on); equal to tile_class 0 and to
    the generic kernel."""
    assert float(OPTS.tile_class) == 1.0
    on = _forms(make(), H, u8=u8)
    assert torch.equal(on["fb"], on["fb_plain"])
    assert torch.equal(on["blk"], on["fb"][3:H - 2]) and (not u8 or torch.equal(on["u8_blk"], on["u8"][3:H - 2]))
    rows = torch.as_tensor(rtx.scene.group_rows(H, 2, 1), device="cuda")
    assert torch.equal(on["grp"], on["fb"][rows])
    monkeypatch.setattr(OPTS, "tile_class", "0")
    _same(on, _forms(make(), H, u8=u8), what + ": tile_class 0")
    monkeypatch.setattr(OPTS, "tile_class", "1")
    monkeypatch.setattr(OPTS, "jit", "0")
    _same(on, _forms(make(), H, jit=False, u8=u8), what + ": generic kernel")
    monkeypatch.setattr(OPTS, "jit", "1")
    return on


@pytest.mark.parametrize("res", SIZES)
def test_two_spheres_plane_every_form(res, monkeypatch):
    ref = oracle_render("TwoSpheresPlane", res, **ONE)
    sc = product_scene("TwoSpheresPlane", res, **ONE)
    img = sc.render()
    sc.jit_wait()
    assert_parity(sc.render(), ref, "TwoSpheresPlane %s tile_class" % (res,))
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    _all_ways(lambda: product_scene("TwoSpheresPlane", res, **ONE), res[1], monkeypatch, "TwoSpheresPlane %s" % (res,))


@pytest.mark.parametrize("name", sorted(constructed()))
def test_constructed_cameras(name, monkeypatch):
    res = SIZES[sorted(constructed()).index(name) % 2]
    d = constructed(res)[name]
    sc = product_scene_dict(d)
    sc.render()
    sc.jit_wait()
    assert_parity(sc.render(), oracle_render_dict(d), name)
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    _all_ways(lambda: product_scene_dict(d), res[1], monkeypatch, name)


@pytest.mark.parametrize("case", range(len(TANGENT_CASES)))
def test_shadow_just_reaching_a_tile(case, monkeypatch):
    """A sphere whose shadow hull touches a tile's corner hit within fp32 rounding
    (shadow_scenes.TANGENT_CASES): the UNSHADOWED flags of the records k_shadow_bins writes on the
    device hold only with their margins. Frames equal the oracle's, tile_class 0 and the generic
    kernel's."""
    d = tangent_scene(case)
    sc = product_scene_dict(d)
    sc.render()
    sc.jit_wait()
    assert_parity(sc.render(), oracle_render_dict(d), "tangent case %d" % case)
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    _all_ways(lambda: product_scene_dict(d), d["resolution"][1], monkeypatch, "tangent case %d" % case)


def _unlike_any(name, k, **edits):
    """Bundled scene `name` with its first sphere's radius changed by a few 1e-4: a scene no other
    test renders, so its kernels (the records are compiled in) are not in memory yet and jit_dump
    speaks for them, whatever frame sizes other tests use."""
    from rtx.io import bundled_scene_dict
    d = bundled_scene_dict(name, resolution=(72, 40))
    d.update(edits)
    ball = next(o for o in d["objects"] if o["type"] == "sphere")
    ball["radius"] = float(ball["radius"]) + 1.37e-4 * k
    return product_scene_dict(d)


def test_the_records_are_built_and_the_kernel_reads_them(monkeypatch, capfd):
    """on == off would also hold with the records silently left out: the specialized kernel must
    be compiled to read them (option jit_dump lists its options) with the option on, and not with
    it off, for a lens camera, or for a scene with secondary rays."""
    monkeypatch.setattr(OPTS, "jit_dump", "1")

    def log_of(sc):
        capfd.readouterr()
        sc.render_device()
        assert sc.jit_wait() == 0
        sc.render_device()
        torch.cuda.synchronize()
        assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
        return capfd.readouterr().err

    assert MACRO in log_of(_unlike_any("TwoSpheresPlane", 1, **ONE))
    err = log_of(_unlike_any("TwoSpheresPlane", 2, AA={"jitter": False, "samples": 2}))
    assert "librtx: jit" in err and "RTX_TILE_CLASS" not in err
    err = log_of(_unlike_any("MirrorRefraction", 3, **ONE))
    assert "librtx: jit" in err and "RTX_TILE_CLASS" not in err
    monkeypatch.setattr(OPTS, "tile_class", "0")
    err = log_of(_unlike_any("TwoSpheresPlane", 4, **ONE))
    assert "librtx: jit" in err and "RTX_TILE_CLASS" not in err


def test_camera_moved_between_frames(monkeypatch):
    """The records belong to the camera: after a move they are rebuilt. Three frames after the
    move equal the oracle's of the moved camera and the frame of tile_class 0."""
    res = (72, 40)
    d = constructed(res)["sphere_at_edge"]
    sc = product_scene_dict(d)
    sc.render_device()
    assert sc.jit_wait() == 0
    before = sc.render_device().clone()
    e = copy.deepcopy(d)
    e["camera"]["position"] = [3.0, 4.0, 6.0]
    e["camera"]["lookAt"] = [0.0, 1.5, 0.0]
    sc.vc.set_camera(e["camera"]["position"], e["camera"]["lookAt"], e["camera"]["up"], e["camera"]["fov"])
    frames = []
    for _ in range(3):
        frames.append(sc.render_device().clone())
        sc.jit_wait()
    assert not torch.equal(before, frames[0])
    ref = oracle_render_dict(e)
    assert_parity(sc.render(), ref, "moved camera")
    monkeypatch.setattr(OPTS, "tile_class", "0")
    sc0 = product_scene_dict(e)
    sc0.render_device()
    assert sc0.jit_wait() == 0
    off = sc0.render_device().clone()
    for f in frames:
        assert torch.equal(f.view(torch.int32), off.view(torch.int32))


def test_sequence_camera(monkeypatch):
    """A sequence camera (one motion time per frame) of the moving sphere: every frame equals
    the sequence with tile_class 0 and the generic kernel's."""
    d = constructed()["moving"]
    d.pop("motion", None)
    times = [0.0, 0.6, 1.2]
    sc = product_scene_dict(d)
    sc.render_sequence(times)
    sc.jit_wait()
    fb = sc.render_sequence(times).clone()
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    assert not torch.equal(fb[0], fb[2])
    monkeypatch.setattr(OPTS, "tile_class", "0")
    sc0 = product_scene_dict(d)
    sc0.render_sequence(times)
    sc0.jit_wait()
    assert torch.equal(sc0.render_sequence(times).view(torch.int32), fb.view(torch.int32))
    monkeypatch.setattr(OPTS, "tile_class", "1")
    monkeypatch.setattr(OPTS, "jit", "0")
    assert torch.equal(product_scene_dict(d).render_sequence(times).view(torch.int32), fb.view(torch.int32))


def test_full_hd_frame(monkeypatch):
    """One 1920x1080 frame of bundled TwoSpheresPlane (the benchmark's) against tile_class 0,
    fp32 with tallies and uint8."""
    res = (1920, 1080)

    def frame():
        sc = product_scene("TwoSpheresPlane", res, **ONE)
        sc.render_device()
        assert sc.jit_wait() == 0
        cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
        fb = sc.render_device(counters=cnt).clone()
        sc.jit_wait()
        plain = sc.render_device().clone()
        assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
        sc.render_device(rgb8=True)
        sc.jit_wait()
        return fb, plain, sc.render_device(rgb8=True).clone(), cnt.cpu().numpy()

    on = frame()
    monkeypatch.setattr(OPTS, "tile_class", "0")
    off = frame()
    assert torch.equal(on[0].view(torch.int32), off[0].view(torch.int32))
    assert torch.equal(on[1].view(torch.int32), on[0].view(torch.int32))
    assert torch.equal(on[2], off[2])
    assert np.array_equal(on[3], off[3]), (on[3], off[3])


def test_scene_outside_the_class(monkeypatch):
    """MirrorRefraction (secondary rays): the same kernel and the same frame, option on and off.
    (A scene of its own, so that no other test's jit_dump finds its kernel in memory.)"""

    def frame():
        sc = _unlike_any("MirrorRefraction", 5, **ONE)
        sc.render_device()
        assert sc.jit_wait() == 0
        return sc.render_device().clone(), sc.last_kernel

    on, kern = frame()
    monkeypatch.setattr(OPTS, "tile_class", "0")
    off, kern0 = frame()
    assert kern == kern0 and kern.startswith("rtx_jit_render_"), (kern, kern0)
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))
