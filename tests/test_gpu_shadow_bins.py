"""Shadow bins on the MI355X (option shadow_bins; rtx_api.hip shadow_bins, k_shadow_bins): the
per-bin occluder masks only skip tests that cannot pass, so a frame with them equals the
frame without them and the oracle's, bit for bit, and so do the ray tallies."""
import copy

import numpy as np
import pytest
import torch

import rtx
from common import OPTS, assert_parity, oracle_render, oracle_render_dict, product_scene, product_scene_dict
from rtx import _native as N
from shadow_scenes import flat_scene

pytestmark = pytest.mark.gpu

ONE = {"AA": {"jitter": False, "samples": 1}}


def _frame(sc):
    """(framebuffer, tallies, kernel) of one frame with the scene-specialized kernel."""
    sc.render_device()
    assert sc.jit_wait() == 0
    cnt = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    fb = sc.render_device(counters=cnt).clone()
    sc.jit_wait()
    fb2 = sc.render_device().clone()  # (the kernel without counters)
    assert torch.equal(fb, fb2)
    return fb, cnt.cpu().numpy(), sc.last_kernel


@pytest.mark.parametrize("res", [(96, 72), (200, 120)])
def test_two_spheres_plane_on_off_oracle(res, monkeypatch):
    ref = oracle_render("TwoSpheresPlane", res, **ONE)
    sc = product_scene("TwoSpheresPlane", res, **ONE)
    img = sc.render()
    sc.jit_wait()
    img = sc.render()
    assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
    assert_parity(img, ref, "TwoSpheresPlane %s shadow_bins 1" % (res,))
    on, cnt_on, kern = _frame(sc)
    assert kern.startswith("rtx_jit_render_"), kern
    monkeypatch.setattr(OPTS, "shadow_bins", "0")
    sc0 = product_scene("TwoSpheresPlane", res, **ONE)
    off, cnt_off, kern0 = _frame(sc0)
    assert kern0.startswith("rtx_jit_render_"), kern0
    assert torch.equal(on, off)
    assert np.array_equal(cnt_on, cnt_off), (cnt_on, cnt_off)
    assert_parity(sc0.render(), ref, "TwoSpheresPlane %s shadow_bins 0" % (res,))


def test_the_table_is_built_and_the_kernel_reads_it(monkeypatch, capfd):
    """on == off == oracle would also hold with the table silently left out. The camera upload
    must run the device build (option setup_log names its step) and the specialized kernel
    must be compiled to read it (option jit_dump lists its options): both with the option on,
    neither with it off or for a lens camera. (A frame size no other test uses: jit_dump
    speaks only for a kernel that is not in memory yet.)"""
    monkeypatch.setattr(OPTS, "setup_log", "1")
    monkeypatch.setattr(OPTS, "jit_dump", "1")
    step, macro, res = "shadow bins (device)", "'-DRTX_SHADOW_BINS=1'", (104, 56)

    def log_of(sc):
        capfd.readouterr()
        sc.render_device()
        assert sc.jit_wait() == 0
        sc.render_device()
        torch.cuda.synchronize()
        assert sc.last_kernel.startswith("rtx_jit_render_"), sc.last_kernel
        return capfd.readouterr().err

    err = log_of(product_scene("TwoSpheresPlane", res, **ONE))
    assert step in err and macro in err
    err = log_of(product_scene("TwoSpheresPlane", res, AA={"jitter": False, "samples": 2}))
    assert "rtx_camera_set" in err and "librtx: jit" in err and step not in err and macro not in err
    monkeypatch.setattr(OPTS, "shadow_bins", "0")
    err = log_of(product_scene("TwoSpheresPlane", res, **ONE))
    assert "rtx_camera_set" in err and "librtx: jit" in err and step not in err and macro not in err


def test_row_blocks_and_row_groups(monkeypatch):
    """A block that starts at row 3 lies off the 8-row grid (its tiles read no bins); an
    interleaved 8-row group does: both equal the rows of the whole frame without the table."""
    res = (200, 120)
    W, H = res
    sc = product_scene("TwoSpheresPlane", res, **ONE)
    sc.render_device()
    assert sc.jit_wait() == 0
    blk = sc.render_device(row0=3, nrows=61).clone()
    grp = sc.render_device(groups=(1, 3)).clone()
    monkeypatch.setattr(OPTS, "shadow_bins", "0")
    sc0 = product_scene("TwoSpheresPlane", res, **ONE)
    sc0.render_device()
    assert sc0.jit_wait() == 0
    full = sc0.render_device().clone()
    assert torch.equal(blk, full[3:64])
    rows = torch.as_tensor(rtx.scene.group_rows(H, 3, 1), device="cuda")
    assert torch.equal(grp, full[rows])


@pytest.mark.parametrize("seed", range(8))
def test_random_point_light_scenes(seed, monkeypatch):
    """Planes and spheres under point lights only: the all-lights-at-once shadow test
    (rtx_trace.h occluded_points) with the masks."""
    d = flat_scene(seed, res=(96, 64), points_only=True)
    ref = oracle_render_dict(d)
    sc = product_scene_dict(d)
    on, cnt_on, kern = _frame(sc)
    assert kern.startswith("rtx_jit_render_"), kern
    assert_parity(sc.render(), ref, "flat_scene %d" % seed)
    monkeypatch.setattr(OPTS, "shadow_bins", "0")
    off, cnt_off, _ = _frame(product_scene_dict(d))
    assert torch.equal(on, off)
    assert np.array_equal(cnt_on, cnt_off)


def test_mixed_lights_boxes_generic_kernel(monkeypatch):
    """Directional lights and boxes (occluded()'s masks), with the specialized and the generic
    kernel."""
    d = flat_scene(4, res=(96, 72))
    ref = oracle_render_dict(d)
    for jit in ("1", "0"):
        monkeypatch.setattr(OPTS, "jit", jit)
        sc = product_scene_dict(d)
        sc.render()
        sc.jit_wait()
        assert_parity(sc.render(), ref, "flat_scene 4 jit=%s" % jit)
        assert sc.last_kernel.startswith("rtx_jit_render_") == (jit == "1"), sc.last_kernel


def test_sequence_with_a_moving_sphere(monkeypatch):
    d = flat_scene(2, res=(96, 72))
    d.pop("motion", None)
    assert any("speed" in o for o in d["objects"])
    times = [0.0, 0.75, 1.5]
    fb = product_scene_dict(d).render_sequence(times).clone()
    for f, t in enumerate(times):
        e = copy.deepcopy(d)
        e["motion"] = {"time": t, "samples": 0, "final": 1}
        got = np.ascontiguousarray(np.transpose(fb[f].cpu().numpy()[::-1], (1, 0, 2))).astype(np.float64)
        assert_parity(got, oracle_render_dict(e), "moving sphere t=%g" % t)
    monkeypatch.setattr(OPTS, "shadow_bins", "0")
    assert torch.equal(product_scene_dict(d).render_sequence(times), fb)
