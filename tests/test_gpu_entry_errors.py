"""The C entry points' argument failures, pinned: the status code and the whole text of
rtx_last_error for each bad call, and which check wins where two faults coincide. The scene is
16 x 8 pixels with one sphere and one light. Every bad call returns from the argument checks:
none of them launches a kernel."""
import ctypes as C

import pytest
import torch

import rtx
from rtx import _native as N
from common import product_scene_dict

pytestmark = pytest.mark.gpu

W, H = 16, 8
INV, STATE = N.RTX_ERR_INVALID, N.RTX_ERR_STATE
NAN, INF = float("nan"), float("inf")


def _scene():
    return product_scene_dict({
        "resolution": [W, H], "AA": {"jitter": False, "samples": 1}, "ambient": [0.1, 0.1, 0.1],
        "camera": {"position": [0.0, 1.0, 4.0], "lookAt": [0.0, 0.5, 0.0], "up": [0.0, 1.0, 0.0], "fov": 50.0},
        "materials": [{"name": "a", "ID": 0, "diffuse": [1, 0, 0], "specular": [0.5, 0.5, 0.5], "hardness": 16}],
        "objects": [{"name": "s", "type": "sphere", "radius": 1.0, "position": [0.0, 0.5, 0.0], "materials": [0]}],
        "lights": [{"name": "l", "type": "point", "position": [2, 5, 3], "colour": [1, 1, 1], "power": 1.0}]})


def _floats(*v):
    return (C.c_float * len(v))(*v)


def _doubles(*v):
    return (C.c_double * len(v))(*v)


def _expect(table):
    lib = N.load()
    for fn, args, code, msg in table:
        assert getattr(lib, fn)(*args) == code, (fn, args, lib.rtx_last_error())
        assert lib.rtx_last_error().decode() == msg, (fn, args)


def test_entry_point_failures():
    sc = _scene()
    h = sc.native().h
    buf = torch.empty(2 * H * W * 3, device="cuda")  # two fp32 frames; the rays and outputs of the cast calls
    p = buf.data_ptr()
    block = H * W * 3 * 4
    up = _floats(0, 0, 1)

    # no camera yet: one entry point of each family
    no_cam = ": rtx_camera_set was not called"
    _expect([
        ("rtx_render", (h, 0, H, p, None, None), STATE, "rtx_render" + no_cam),
        ("rtx_render_groups", (h, 0, 1, p, None, None), STATE, "rtx_render_groups" + no_cam),
        ("rtx_render_frames", (h, 0, H, p, 0, 2, block, None, None), STATE, "rtx_render_frames" + no_cam),
        ("rtx_render_sequence", (h, 0, H, p, 0, 0, 1, block, None, None), STATE, "rtx_render_sequence" + no_cam),
        ("rtx_render_aov", (h, 0, H, 0, p, None, None, None, None, None, None), STATE, "rtx_render_aov" + no_cam),
        ("rtx_render_occlusion", (h, 0, H, 0, p, None, None, 0, INF, None), STATE, "rtx_render_occlusion" + no_cam),
    ])

    sc._set_camera(0, 1)  # the ordinary camera: one window
    rows = ": row range outside the image"
    overlap = ": need 1 <= nframes <= 65535 and frames that do not overlap"
    null_fb = ": null framebuffer"
    phase = ": need 0 <= phase < stride"
    aov_null = (None,) * 7
    dirs65 = _floats(*([0.0, 0.0, 1.0] * 65))
    T = N.RTX_CAST_MAX_TIMES
    _expect([
        ("rtx_render", (h, 0, H + 1, p, None, None), INV, "rtx_render" + rows),
        ("rtx_render", (h, -1, 2, p, None, None), INV, "rtx_render" + rows),
        ("rtx_render", (h, 0, H, None, None, None), INV, "rtx_render" + null_fb),
        ("rtx_render_groups", (h, 2, 2, p, None, None), INV, "rtx_render_groups" + phase),
        ("rtx_render_groups", (h, 0, 0, p, None, None), INV, "rtx_render_groups" + phase),
        ("rtx_render_groups", (h, 0, 1, None, None, None), INV, "rtx_render_groups" + null_fb),
        ("rtx_render_frames", (h, 4, H - 3, p, 0, 2, block, None, None), INV, "rtx_render_frames" + rows),
        ("rtx_render_frames", (h, 0, H, p, 0, 2, block - 4, None, None), INV, "rtx_render_frames" + overlap),
        ("rtx_render_frames", (h, 0, H, p, 0, 0, block, None, None), INV, "rtx_render_frames" + overlap),
        ("rtx_render_frames", (h, 0, H, None, 0, 2, block, None, None), INV, "rtx_render_frames" + null_fb),
        ("rtx_render_groups_frames", (h, 3, 2, p, 0, 2, block, None, None), INV, "rtx_render_groups_frames" + phase),
        ("rtx_render_sequence", (h, 0, H, p, 0, 1, 1, block, None, None), INV,
         "rtx_render_sequence: frames [1, 2) outside the camera's sequence of 1"),
        ("rtx_render_sequence", (h, 0, H, p, 0, -1, 1, block, None, None), INV, "rtx_render_sequence: frame0 < 0"),
        # rtx_render_aov
        ("rtx_render_aov", (h, 0, H) + (0,) + aov_null, INV,
         "rtx_render_aov: no buffer requested (all six pointers are null)"),
        ("rtx_render_aov", (h, 0, H, 1, p, None, None, None, None, None, None), INV,
         "rtx_render_aov: frame 1 outside the camera's 1 window(s)"),
        ("rtx_render_aov", (h, 1, H, 0, p, None, None, None, None, None, None), INV, "rtx_render_aov" + rows),
        ("rtx_render_aov", (h, 0, H + 1, 0) + aov_null, INV, "rtx_render_aov" + rows),  # the rows come first
        # rtx_render_occlusion
        ("rtx_render_occlusion", (h, 0, H, 0, None, None, up, 1, INF, None), INV,
         "rtx_render_occlusion: no buffer requested (both pointers are null)"),
        ("rtx_render_occlusion", (h, 0, H, 0, None, p, up, 0, INF, None), INV,
         "rtx_render_occlusion: 1 to 64 ambient-occlusion directions, got 0"),
        ("rtx_render_occlusion", (h, 0, H, 0, None, p, dirs65, 65, INF, None), INV,
         "rtx_render_occlusion: 1 to 64 ambient-occlusion directions, got 65"),
        ("rtx_render_occlusion", (h, 0, H, 0, None, p, _floats(0, 0, 1, 0, INF, 1), 2, INF, None), INV,
         "rtx_render_occlusion: direction 1 is not finite"),
        ("rtx_render_occlusion", (h, 0, H, 0, None, p, up, 1, 0.0, None), INV,
         "rtx_render_occlusion: ao_radius must be > 0 or +inf"),
        ("rtx_render_occlusion", (h, 0, H, 0, None, p, up, 1, NAN, None), INV,
         "rtx_render_occlusion: ao_radius must be > 0 or +inf"),
        ("rtx_render_occlusion", (h, 2, H, 0, p, None, None, 0, INF, None), INV, "rtx_render_occlusion" + rows),
        ("rtx_render_occlusion", (h, 0, H, 1, p, None, None, 0, INF, None), INV,
         "rtx_render_occlusion: frame 1 outside the camera's 1 window(s)"),
        # (no rows would be no work, but the directions are checked first)
        ("rtx_render_occlusion", (h, 3, 0, 0, None, p, up, 0, INF, None), INV,
         "rtx_render_occlusion: 1 to 64 ambient-occlusion directions, got 0"),
        # rtx_cast_rays
        ("rtx_cast_rays", (h, 4, p, p, _doubles(0.0), 1, 3, p, None, None), INV,
         "rtx_cast_rays: group 3 must be >= 1 and divide n = 4"),
        ("rtx_cast_rays", (h, 4, p, p, _doubles(0.0), 1, 0, p, None, None), INV,
         "rtx_cast_rays: group 0 must be >= 1 and divide n = 4"),
        ("rtx_cast_rays", (h, 4, p, p, _doubles(0.0), 0, 1, p, None, None), INV,
         "rtx_cast_rays: 1 to %d motion times, got 0" % T),
        ("rtx_cast_rays", (h, 4, p, p, _doubles(0.0, NAN), 2, 1, p, None, None), INV,
         "rtx_cast_rays: motion time 1 is not finite"),
        ("rtx_cast_rays", (h, 4, p, p, _doubles(1e300), 1, 1, p, None, None), INV,
         "rtx_cast_rays: motion time 0 is not finite"),
        ("rtx_cast_rays", (h, 4, None, p, _doubles(0.0), 1, 1, p, None, None), INV,
         "rtx_cast_rays: null rays or null output"),
    ])

    sc._set_camera(0, 1, rtx.frame_windows(0, 1, 2))  # a sequence camera: two windows
    _expect([
        ("rtx_render_sequence", (h, 0, H, p, 0, 1, 2, block, None, None), INV,
         "rtx_render_sequence: frames [1, 3) outside the camera's sequence of 2"),
        ("rtx_render_sequence", (h, 0, H + 1, p, 0, 0, 2, block, None, None), INV, "rtx_render_sequence" + rows),
        ("rtx_render_sequence", (h, 0, H, p, 0, 0, 2, block - 4, None, None), INV, "rtx_render_sequence" + overlap),
        ("rtx_render_sequence", (h, 0, H, None, 0, 0, 2, block, None, None), INV, "rtx_render_sequence" + null_fb),
        ("rtx_render_groups_sequence", (h, 1, 1, p, 0, 0, 2, block, None, None), INV,
         "rtx_render_groups_sequence" + phase),
        ("rtx_render_aov", (h, 0, H, 2, p, None, None, None, None, None, None), INV,
         "rtx_render_aov: frame 2 outside the camera's 2 window(s)"),
        ("rtx_render_occlusion", (h, 0, H, -1, p, None, None, 0, INF, None), INV,
         "rtx_render_occlusion: frame -1 outside the camera's 2 window(s)"),
    ])
    assert sc.last_kernel == ""  # nothing was launched
