"""The primary-ray direction table on the MI355X (rtx_kernels.h ray_slot / k_ray_dirs; option
ray_table): a one-sample, unjittered camera's scene-specialized kernel reads each pixel's
direction from the table rtx_camera_set filled. Its frames equal, as uint32 words, the frames
with ray_table 0 (the kernel computes the direction), the generic kernel's (jit 0) and the
oracle's: in frames of one pixel, one tile, ragged tiles and several blocks, in every launch
form, after a camera move and after size changes that regrow and reuse the buffer. Cameras
outside the class (jitter, a lens, several samples), scenes with secondary rays or a mesh
without face boxes (unless option ray_table is 4) and tables over ray_table_max_mb get no RTX_RAY_TABLE kernel."""
import copy

import numpy as np
import pytest
import torch

import rtx
import uniform_scenes as U
from common import OPTS, oracle_render_dict, product_scene_dict
from rtx.io import bundled_scene_dict

pytestmark = pytest.mark.gpu

DEFINE = "-DRTX_RAY_TABLE="
CAMERA = ([0.3, 2.0, 2.5], [0.0, 1.0, -0.5], [0.0, 1.0, 0.0], 60.0)  # U.tsp's
MOVED = ([1.5, 3.0, 7.0], [0.0, 0.5, 0.0], [0.0, 1.0, 0.0], 40.0)


def _bits(img):
    return np.ascontiguousarray(np.asarray(img, np.float32)).view(np.uint32)


def _specialized(sc, **kw):
    sc.render_device(**kw)
    assert sc.jit_wait() == 0
    sc.render_device(**kw)
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    return sc


def _frame(d, monkeypatch=None, **opts):
    """The frame of a fresh scene of d, rendered with the options (ray_table, jit) set."""
    for k, v in opts.items():
        monkeypatch.setattr(OPTS, k, v)
    sc = product_scene_dict(d)
    if opts.get("jit") == "0":
        fb = sc.render_device().clone()
        assert sc.last_kernel.startswith("k_render"), sc.last_kernel
    else:
        fb = _specialized(sc).render_device().clone()
    for k in opts:
        monkeypatch.setattr(OPTS, k, "1")  # (the default of both)
    return fb


def _jit_options(d, capfd, monkeypatch):
    """The hiprtc option line of the kernel the library compiles for d (option jit_dump, which
    speaks for a kernel that is not in memory yet: frame widths no other test here uses), and
    the frame."""
    monkeypatch.setattr(OPTS, "jit_dump", "1")
    capfd.readouterr()
    sc = _specialized(product_scene_dict(d))
    fb = sc.render_device().clone()
    err = capfd.readouterr().err
    head = "librtx: jit %s:" % sc.last_kernel.split("+")[0]
    at = err.find(head)
    assert at >= 0, "no jit_dump of %s in:\n%s" % (sc.last_kernel, err[:2000])
    return err[at:].partition("\n")[0], fb


# 1x1, one whole tile, ragged tiles in both directions, several tiles, more than one block
@pytest.mark.parametrize("res", [(1, 1), (8, 8), (9, 7), (67, 45), (130, 9)])
def test_sizes_equal_option_off_generic_and_oracle(res, monkeypatch):
    d = U.tsp(res)
    on = _frame(d)
    assert torch.equal(on.view(torch.int32), _frame(d, monkeypatch, ray_table="0").view(torch.int32))
    assert torch.equal(on.view(torch.int32), _frame(d, monkeypatch, jit="0").view(torch.int32))
    sc = _specialized(product_scene_dict(d))
    assert np.array_equal(_bits(sc.render()), _bits(oracle_render_dict(d)))


@pytest.mark.parametrize("name", ["TwoSpheresPlane", "MirrorRefraction", "TorusMesh"])
def test_scenes(name, monkeypatch):
    d = U.bundled(name, (67, 45))
    on = _frame(d)
    # (MirrorRefraction gets the table only on request: secondary rays measured slower with it;
    # TorusMesh at this size has heavy tiles, whose pass computes its own rays)
    assert torch.equal(on.view(torch.int32), _frame(d, monkeypatch, ray_table="4").view(torch.int32))
    assert torch.equal(on.view(torch.int32), _frame(d, monkeypatch, ray_table="0").view(torch.int32))
    assert torch.equal(on.view(torch.int32), _frame(d, monkeypatch, jit="0").view(torch.int32))
    sc = _specialized(product_scene_dict(d))
    assert np.array_equal(_bits(sc.render()), _bits(oracle_render_dict(d)))
    # (TorusMesh and MirrorRefraction: the measured tile order's whole-frame launches too)
    for _ in range(3):
        assert torch.equal(sc.render_device(), on)


def test_the_class_gets_the_define(capfd, monkeypatch):
    assert DEFINE + "1" in _jit_options(U.tsp((59, 21)), capfd, monkeypatch)[0]
    assert DEFINE + "1" in _jit_options(U.bundled("TorusMesh", (59, 21)), capfd, monkeypatch)[0]


def test_secondary_rays_get_the_define_on_request_only(capfd, monkeypatch):
    d = U.bundled("MirrorRefraction", (59, 21))
    line, off = _jit_options(d, capfd, monkeypatch)
    assert DEFINE not in line
    monkeypatch.setattr(OPTS, "ray_table", "4")
    line, on = _jit_options(d, capfd, monkeypatch)
    assert DEFINE + "1" in line
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))


def test_mesh_without_face_boxes_on_request(tmp_path, capfd, monkeypatch):
    """The mesh corpus' 5,120-face blob (heavy tiles, no face boxes): no table by default."""
    import meshgen
    d = meshgen.corpus_scene("blob4", meshgen.corpus(tmp_path), res=(59, 37))
    d["AA"] = {"jitter": False, "samples": 1}
    line, off = _jit_options(d, capfd, monkeypatch)
    assert DEFINE not in line
    monkeypatch.setattr(OPTS, "ray_table", "4")
    line, on = _jit_options(d, capfd, monkeypatch)
    assert DEFINE + "1" in line
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))


def test_launch_forms(monkeypatch):
    """Row blocks off the 8-row grid, interleaved groups, a column strip, the uint8 output."""
    res = (67, 45)
    d = U.tsp(res)
    sc = _specialized(product_scene_dict(d))
    full = sc.render_device().clone()
    assert torch.equal(sc.render_device(row0=3, nrows=13), full[3:16])
    assert torch.equal(sc.render_device(row0=40, nrows=5), full[40:45])
    rows = torch.as_tensor(rtx.scene.group_rows(res[1], 3, 1), device="cuda")
    assert torch.equal(sc.render_device(groups=(1, 3)), full[rows])
    sc.render_device(rgb8=True)
    sc.jit_wait()
    u8 = sc.render_device(rgb8=True)
    assert sc.last_kernel.endswith("_rgb8"), sc.last_kernel
    assert torch.equal(u8, (full.double() * 255.0).to(torch.int32).to(torch.uint8))
    assert torch.equal(sc.render_device(row0=3, nrows=13, rgb8=True), u8[3:16])
    strip = _specialized(product_scene_dict(d), subimage=1, tasks=2)
    img = strip.render(subimage=1, tasks=2)
    assert strip.last_kernel.startswith("rtx_jit_render_"), strip.last_kernel
    assert np.array_equal(_bits(img), _bits(oracle_render_dict(d, 1, 2)))
    monkeypatch.setattr(OPTS, "ray_table", "0")
    off = _specialized(product_scene_dict(d), subimage=1, tasks=2)
    assert torch.equal(off.render_device(subimage=1, tasks=2), strip.render_device(subimage=1, tasks=2))


def test_sequence_camera_three_motion_times(monkeypatch):
    d = U.scenes((67, 45))["moving"]
    d.pop("motion")
    times = [0.0, 0.6, 1.25]
    sc = product_scene_dict(d)
    sc.render_sequence(times)
    assert sc.jit_wait() == 0
    fb = sc.render_sequence(times).clone()
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    monkeypatch.setattr(OPTS, "ray_table", "0")
    off = product_scene_dict(d)
    off.render_sequence(times)
    assert off.jit_wait() == 0
    assert torch.equal(off.render_sequence(times).view(torch.int32), fb.view(torch.int32))
    for f, t in enumerate(times):
        e = copy.deepcopy(d)
        e["motion"] = {"time": t, "samples": 0, "final": 1}
        got = np.ascontiguousarray(np.transpose(fb[f].cpu().numpy()[::-1], (1, 0, 2)))
        assert np.array_equal(_bits(got), _bits(oracle_render_dict(e))), t


def test_side_stream_render_right_after_a_move():
    """rtx_camera_set fills the table on the null stream and does not wait for it; a render on a
    non-blocking stream, which has no order of its own with the null stream, must still come
    after the fill. A full-size frame, so the fill takes as long as a launch does; the moved
    camera's kernel is already in memory, so nothing else delays the render."""
    res = (1920, 1080)
    d = U.tsp(res)
    sc = _specialized(product_scene_dict(d))
    side = torch.cuda.Stream()
    out = torch.empty((res[1], res[0], 3), dtype=torch.float32, device="cuda")
    for k in range(3):
        eye = [MOVED[0][0] + 0.25 * k, MOVED[0][1], MOVED[0][2]]
        fresh = product_scene_dict(d)
        fresh.vc.set_camera(eye, *MOVED[1:])
        want = _specialized(fresh).render_device().clone()
        torch.cuda.synchronize()
        sc.vc.set_camera(eye, *MOVED[1:])
        sc.render_device(out=out, stream=side)  # (the upload, the fill and the frame in one call)
        assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
        side.synchronize()
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), k


def test_moved_camera():
    """Render, move, render: the second upload's table, not the first's."""
    d = U.tsp((67, 45))
    sc = _specialized(product_scene_dict(d))
    first = sc.render_device().clone()
    sc.vc.set_camera(*MOVED)
    moved = _specialized(sc).render_device().clone()
    assert not torch.equal(moved, first)
    fresh = product_scene_dict(d)
    fresh.vc.set_camera(*MOVED)
    assert torch.equal(_specialized(fresh).render_device(), moved)
    sc.vc.set_camera(*CAMERA)
    assert torch.equal(_specialized(sc).render_device(), first)


def test_size_up_down_up():
    """The buffer regrown (67x45 -> 130x90), reused for a smaller table and for the larger again."""
    sc = product_scene_dict(U.tsp((67, 45)))
    for res in [(67, 45), (130, 90), (9, 7), (130, 90)]:
        sc.vc.set_viewport(*res)
        sc.vc.set_camera(*CAMERA)
        got = _specialized(sc).render_device().clone()
        assert tuple(got.shape) == (res[1], res[0], 3)
        assert torch.equal(got, _specialized(product_scene_dict(U.tsp(res))).render_device()), res


@pytest.mark.parametrize("kind", ["jitter", "lens", "samples"])
def test_cameras_outside_the_class_get_no_define(kind, capfd, monkeypatch):
    if kind == "lens":  # (the bundled scene's own lens and samples)
        d = bundled_scene_dict("DepthOfField", resolution=[44, 24])
        d.pop("__base_dir__", None)
    else:
        d = U.tsp((61, 21) if kind == "jitter" else (62, 21))
        d["AA"] = {"jitter": True, "samples": 1} if kind == "jitter" else {"jitter": False, "samples": 4}
    assert DEFINE not in _jit_options(d, capfd, monkeypatch)[0]


def test_table_over_the_cap_falls_back(capfd, monkeypatch):
    d = U.tsp((131, 9))  # 17 x 2 tiles x 768 B = 26112 B
    monkeypatch.setattr(OPTS, "ray_table_max_mb", "0.02")  # 20971 B
    line, capped = _jit_options(d, capfd, monkeypatch)
    assert DEFINE not in line
    monkeypatch.setattr(OPTS, "ray_table_max_mb", "0.025")  # 26214 B
    line, on = _jit_options(d, capfd, monkeypatch)
    assert DEFINE in line
    assert torch.equal(on.view(torch.int32), capped.view(torch.int32))


def test_aovs_and_occlusion_unchanged(monkeypatch):
    """(The first-hit passes compute their rays themselves: the option must leave them alone.)"""
    d = U.bundled("TorusMesh", (67, 45))
    sc = _specialized(product_scene_dict(d))
    aov_on, occ_on = sc.render_aovs(), sc.render_occlusion(ao_samples=4)
    monkeypatch.setattr(OPTS, "ray_table", "0")
    sc2 = _specialized(product_scene_dict(d))
    aov_off, occ_off = sc2.render_aovs(), sc2.render_occlusion(ao_samples=4)
    for on, off in ((aov_on, aov_off), (occ_on, occ_off)):
        assert set(on) == set(off)
        for k in on:
            assert torch.equal(on[k].contiguous().view(torch.uint8), off[k].contiguous().view(torch.uint8)), k
