"""Wave-uniform hits on the MI355X (rtx_trace.h cast_ray / shade_uniform<K>; option uniform_hit):
the scene-specialized kernel with the per-object shading copies renders the oracle's frame, the
generic kernel's (jit 0) and its own with uniform_hit 0, bit for bit (uint32 words), in tiny
frames of whole tiles and with edge tiles -- where a wave's first lanes may be outside the frame
or have missed -- and in every launch form; the ray tallies equal the generic kernel's."""
import numpy as np
import pytest
import torch

import rtx
import uniform_scenes as U
from common import OPTS, oracle_render_dict, product_scene_dict
from rtx import _native as N

pytestmark = pytest.mark.gpu


def _bits(img):
    return np.ascontiguousarray(np.asarray(img, np.float32)).view(np.uint32)


def _specialized(sc):
    sc.render_device()
    assert sc.jit_wait() == 0
    sc.render_device()
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    return sc


def _frame_and_tallies(sc):
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    sc.render_device(counters=cnt)
    sc.jit_wait()
    fb = sc.render_device(counters=cnt.zero_()).clone()
    return fb, cnt.cpu().numpy()


def _three_ways(d, monkeypatch):
    """(scene with uniform_hit on, its frame, tallies); asserts frame and tallies equal those
    with uniform_hit 0 and of the generic kernel."""
    sc = _specialized(product_scene_dict(d))
    fb, cnt = _frame_and_tallies(sc)
    assert torch.equal(sc.render_device(), fb)  # (the kernel without counters)
    monkeypatch.setattr(OPTS, "uniform_hit", "0")
    off, off_cnt = _frame_and_tallies(_specialized(product_scene_dict(d)))
    monkeypatch.setattr(OPTS, "uniform_hit", "1")
    monkeypatch.setattr(OPTS, "jit", "0")
    g = product_scene_dict(d)
    gen, gen_cnt = _frame_and_tallies(g)
    assert g.last_kernel.startswith("k_render"), g.last_kernel
    monkeypatch.setattr(OPTS, "jit", "1")
    for other, oc, what in ((off, off_cnt, "uniform_hit 0"), (gen, gen_cnt, "generic")):
        assert torch.equal(fb.view(torch.int32), other.view(torch.int32)), what
        assert np.array_equal(cnt[:12], oc[:12]), (what, cnt, oc)
    return sc, fb, cnt


SCENES = ["tsp", "both_unlit", "one_material", "zero_diffuse_specular", "negative_zero_diffuse", "negative_light",
          "light_on_plane", "directional", "box", "over_cap", "moving"]


CASES = [(n, U.RES[0]) for n in SCENES] + [(n, U.RES[1]) for n in ("tsp", "light_on_plane", "box")]


@pytest.fixture(scope="module")
def scene_dicts():
    return {r: U.scenes(r) for r in U.RES}


@pytest.mark.parametrize("name,res", CASES)
def test_scenes_equal_oracle_generic_and_option_off(scene_dicts, name, res, monkeypatch):
    d = scene_dicts[res][name]
    sc, fb, cnt = _three_ways(d, monkeypatch)
    ref, tl = oracle_render_dict(d, tallies=True)
    assert np.array_equal(_bits(sc.render()), _bits(ref)), name
    assert list(cnt[:10]) == tl[:10] and cnt[10] == tl[11] and cnt[11] == tl[12]


@pytest.mark.parametrize("name,res", [("MirrorRefraction", (64, 36)), ("TorusMesh", (48, 48))])
def test_secondary_rays_and_mesh(name, res, monkeypatch):
    """TorusMesh shades its plane by the copy and its mesh hits per lane. MirrorRefraction keeps
    cast_ray's loop: kernels with secondary rays get no dispatch (the copies built through the
    chain loop slowed mr1080 by 7 %), so its case only shows that the option
    leaves that kernel's frames alone."""
    d = U.bundled(name, res)
    sc, fb, _ = _three_ways(d, monkeypatch)
    assert np.array_equal(_bits(sc.render()), _bits(oracle_render_dict(d))), name


@pytest.mark.parametrize("res", U.RES)
def test_launch_forms(res):
    """Row blocks off the tile grid, groups, uint8 output and a column strip of TwoSpheresPlane."""
    W, H = res
    d = U.tsp(res)
    sc = _specialized(product_scene_dict(d))
    full = sc.render_device().clone()
    assert torch.equal(sc.render_device(row0=3, nrows=13), full[3:16])
    rows = torch.as_tensor(rtx.scene.group_rows(H, 2, 1), device="cuda")
    assert torch.equal(sc.render_device(groups=(1, 2)), full[rows])
    sc.render_device(rgb8=True)
    sc.jit_wait()
    u8 = sc.render_device(rgb8=True)
    assert sc.last_kernel.endswith("_rgb8"), sc.last_kernel
    assert torch.equal(u8, (full.double() * 255.0).to(torch.int32).to(torch.uint8))
    strip = product_scene_dict(d)
    strip.render(subimage=1, tasks=2)
    assert strip.jit_wait() == 0
    img = strip.render(subimage=1, tasks=2)
    assert strip.last_kernel.startswith("rtx_jit_render_"), strip.last_kernel
    assert np.array_equal(_bits(img), _bits(oracle_render_dict(d, 1, 2)))


def test_sequence_camera():
    """Two windows of motion times of the moving-sphere scene."""
    import copy
    d = U.scenes(U.RES[1])["moving"]
    d.pop("motion")
    times = [0.0, 1.25]
    fb = product_scene_dict(d).render_sequence(times).clone()
    for f, t in enumerate(times):
        e = copy.deepcopy(d)
        e["motion"] = {"time": t, "samples": 0, "final": 1}
        got = np.ascontiguousarray(np.transpose(fb[f].cpu().numpy()[::-1], (1, 0, 2)))
        assert np.array_equal(_bits(got), _bits(oracle_render_dict(e))), t


def test_aovs_and_cast_rays_unchanged(monkeypatch):
    """render_aovs and cast_rays with uniform_hit on and off: the same buffers."""
    d = U.tsp(U.RES[1])
    sc = _specialized(product_scene_dict(d))
    on = sc.render_aovs()
    o, dr, _ = U.primary_rays(sc)
    rays_on = sc.cast_rays(o, dr)
    monkeypatch.setattr(OPTS, "uniform_hit", "0")
    sc2 = _specialized(product_scene_dict(d))
    off = sc2.render_aovs()
    rays_off = sc2.cast_rays(o, dr)
    assert set(on) == set(off)
    for k in on:
        assert torch.equal(on[k].contiguous().view(torch.uint8), off[k].contiguous().view(torch.uint8)), k
    assert np.array_equal(_bits(rays_on), _bits(rays_off))
