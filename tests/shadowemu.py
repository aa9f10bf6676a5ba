"""Tests-only harness for the shadow bins (tests/native/rtx_shadowemu.hip): the host
emulation plus the table rtx_camera_set builds, its check against the device's own
occlusion test and a render that reads it."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostemu

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rtx_shadowemu.hip")
LIB = os.path.join(HERE, "native", "librtx_shadowemu.so")
DEPS = [SRC] + hostemu.DEPS

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in DEPS):
            subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fopenmp",
                                   "-fPIC", "-shared", "-o", LIB, SRC, "-lhiprtc"])
        _lib = C.CDLL(LIB)
        vp = C.c_void_p
        _lib.rtx_shadowemu_masks.argtypes = [vp, vp, C.c_double, vp, C.c_int64, C.c_int, vp]
        _lib.rtx_shadowemu_masks.restype = C.c_int64
        _lib.rtx_shadowemu_check.argtypes = [vp, vp, vp, vp]
        _lib.rtx_shadowemu_render.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp]
        _lib.rtx_hostemu_last_error.restype = C.c_char_p
    return _lib


def _chk(rc):
    if rc != 0:
        raise RuntimeError("shadowemu failed %d: %s" % (rc, lib().rtx_hostemu_last_error().decode()))


def masks(scene, subimage=0, tasks=1, margin=1.0, reps=1):
    """The camera's shadow bins: (uint32 [bins_y, bins_x, n_lights], host ms of the build), or
    None when the camera gets none."""
    sd = scene.scene_desc()
    cd, tables = scene.camera_desc(subimage, tasks)
    bx, by = (cd.ncols + 7) // 8, (cd.height + 7) // 8
    out = np.zeros(bx * by * sd.n_lights, np.uint32)
    ms = C.c_double(0.0)
    n = lib().rtx_shadowemu_masks(C.addressof(sd), C.addressof(cd), margin, out.ctypes.data, out.size, reps, C.addressof(ms))
    if n == 0:
        return None
    assert n == out.size, (n, out.size)
    return out.reshape(by, bx, sd.n_lights), ms.value


def check(scene, table, subimage=0, tasks=1):
    """(occluding single-object tests, those whose bit is clear in ``table``, level-0 hits) over
    every pixel, light, sphere and box."""
    sd = scene.scene_desc()
    cd, tables = scene.camera_desc(subimage, tasks)
    t = np.ascontiguousarray(table, np.uint32)
    res = np.zeros(3, np.int64)
    _chk(lib().rtx_shadowemu_check(C.addressof(sd), C.addressof(cd), t.ctypes.data, res.ctypes.data))
    return int(res[0]), int(res[1]), int(res[2])


def render(scene, use_masks, subimage=0, tasks=1, threads=8):
    """hostemu.render's result with the shadow bins read (use_masks) or not, and whether the
    frame had a table: (image, counters, bound)."""
    sd = scene.scene_desc()
    cd, tables = scene.camera_desc(subimage, tasks)
    H = scene.vc.height
    fb = np.zeros((H, cd.ncols, 3), np.float32)
    cnt = np.zeros(16, np.uint64)
    bound = C.c_int(0)
    _chk(lib().rtx_shadowemu_render(C.addressof(sd), C.addressof(cd), 1 if use_masks else 0, fb.ctypes.data,
                                    cnt.ctypes.data, threads, C.addressof(bound)))
    img = np.ascontiguousarray(np.transpose(fb[::-1], (1, 0, 2))).astype(np.float64)
    return img, cnt, bool(bound.value)
