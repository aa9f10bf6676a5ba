"""Tests-only harness for the tile classes (tests/native/rtx_classemu.hip): the host
emulation plus the class records rtx_camera_set builds, their check at every pixel against the
device's own hit and occlusion tests, and renders that read them (this library's own copy of
the option tile_class)."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostemu

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rtx_classemu.hip")
LIB = os.path.join(HERE, "native", "librtx_classemu.so")
DEPS = [SRC] + hostemu.DEPS

SKY, PLANE, UNSHADOWED = 1, 2, 4

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in DEPS):
            subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fopenmp",
                                   "-fPIC", "-shared", "-o", LIB, SRC, "-lhiprtc"])
        _lib = C.CDLL(LIB)
        vp = C.c_void_p
        _lib.rtx_classemu_records.argtypes = [vp, vp, C.c_double, C.c_double, vp, C.c_int64]
        _lib.rtx_classemu_records.restype = C.c_int64
        _lib.rtx_classemu_bound.argtypes = [vp, vp, vp, C.c_int64]
        _lib.rtx_classemu_bound.restype = C.c_int64
        _lib.rtx_classemu_check.argtypes = [vp, vp, vp, vp]
        _lib.rtx_hostemu_render.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, vp, C.c_int]
        _lib.rtx_hostemu_render_rows.argtypes = [vp, vp, vp, C.c_int32, vp, C.c_int]
        _lib.rtx_set_option.argtypes = [C.c_char_p, C.c_char_p]
        _lib.rtx_hostemu_last_error.restype = C.c_char_p
    return _lib


def _chk(rc):
    if rc != 0:
        raise RuntimeError("classemu failed %d: %s" % (rc, lib().rtx_hostemu_last_error().decode()))


def set_option(name, value):
    _chk(lib().rtx_set_option(str(name).encode(), str(value).encode()))


def _shape(scene, subimage, tasks):
    sd = scene.scene_desc()
    cd, tables = scene.camera_desc(subimage, tasks)
    return sd, cd, tables, (cd.ncols + 7) // 8, (cd.height + 7) // 8


def records(scene, subimage=0, tasks=1, margin=1.0, cls_rho=1.0):
    """The camera's class records, uint32 [bins_y, bins_x, 2] = (object mask, class word), or
    None when the camera gets none. margin, cls_rho: the test knobs (1 = the product's)."""
    sd, cd, tables, bx, by = _shape(scene, subimage, tasks)
    out = np.zeros(bx * by * 2, np.uint32)
    n = lib().rtx_classemu_records(C.addressof(sd), C.addressof(cd), margin, cls_rho, out.ctypes.data, out.size)
    assert n >= 0, lib().rtx_hostemu_last_error().decode()
    if n == 0:
        return None
    assert n == bx * by, (n, bx, by)
    return out.reshape(by, bx, 2)


def bound(scene, subimage=0, tasks=1):
    """The records in the camera's own table (what a render reads), or None."""
    sd, cd, tables, bx, by = _shape(scene, subimage, tasks)
    out = np.zeros(bx * by * 2, np.uint32)
    n = lib().rtx_classemu_bound(C.addressof(sd), C.addressof(cd), out.ctypes.data, out.size)
    assert n >= 0, lib().rtx_hostemu_last_error().decode()
    if n == 0:
        return None
    return out.reshape(by, bx, 2)


def check(scene, rec, subimage=0, tasks=1):
    """Every flag of ``rec`` at every pixel: dict of sky (pixels, wrong), plane (pixels, wrong),
    unshadowed ((pixel, light) tests, occluded)."""
    sd, cd, tables, bx, by = _shape(scene, subimage, tasks)
    r = np.ascontiguousarray(rec, np.uint32)
    assert r.size == bx * by * 2
    res = np.zeros(6, np.int64)
    _chk(lib().rtx_classemu_check(C.addressof(sd), C.addressof(cd), r.ctypes.data, res.ctypes.data))
    res = [int(x) for x in res]
    return {"sky": (res[0], res[1]), "plane": (res[2], res[3]), "unshadowed": (res[4], res[5])}


def render(scene, subimage=0, tasks=1, threads=8):
    """hostemu.render with this library: (float32 [H, W, 3] framebuffer rows top first, counters)."""
    sd, cd, tables, bx, by = _shape(scene, subimage, tasks)
    H = scene.vc.height
    fb = np.zeros((H, cd.ncols, 3), np.float32)
    cnt = np.zeros(16, np.uint64)
    _chk(lib().rtx_hostemu_render(C.addressof(sd), C.addressof(cd), 0, H, fb.ctypes.data, cnt.ctypes.data, threads))
    return fb, cnt


def render_block(scene, row0, nrows, threads=8):
    """Rows [row0, row0 + nrows) as one contiguous block launch: (framebuffer, counters)."""
    sd, cd, tables, bx, by = _shape(scene, 0, 1)
    fb = np.zeros((nrows, cd.ncols, 3), np.float32)
    cnt = np.zeros(16, np.uint64)
    _chk(lib().rtx_hostemu_render(C.addressof(sd), C.addressof(cd), row0, nrows, fb.ctypes.data, cnt.ctypes.data, threads))
    return fb, cnt


def render_rows(scene, rows, threads=8):
    """The packed image rows ``rows`` (an interleaved-group launch): framebuffer."""
    sd, cd, tables, bx, by = _shape(scene, 0, 1)
    rows = np.ascontiguousarray(np.asarray(rows, np.int32))
    fb = np.zeros((len(rows), cd.ncols, 3), np.float32)
    _chk(lib().rtx_hostemu_render_rows(C.addressof(sd), C.addressof(cd), rows.ctypes.data, len(rows), fb.ctypes.data, threads))
    return fb
