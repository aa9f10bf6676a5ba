"""The primary-ray direction table in the host emulation (rtx_api.hip CamTables::rays,
rtx_kernels.h ray_slot / ray_table_entry; option ray_table): the table a camera gets holds
primary_dir of every pixel at the pixel's tile-major slot, frames rendered through it equal the
frames that compute the direction per pixel, byte for byte, and jit_spec hands RTX_RAY_TABLE to
exactly the one-sample, unjittered cameras of flat scenes without secondary rays or meshes
without face boxes whose table fits ray_table_max_mb."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostemu
import meshgen
import uniform_scenes as U
from common import OPTS, product_scene, product_scene_dict
from jitspec import jit_spec

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rtx_hostemu_rays.hip")
LIB = os.path.join(HERE, "native", "librtx_hostemu_rays.so")
DEFINE = "-DRTX_RAY_TABLE=1"


@pytest.fixture(scope="module")
def rays():
    """The host emulation with the table's two entry points (tests/native/rtx_hostemu_rays.hip)."""
    deps = hostemu.DEPS + [SRC]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fopenmp",
                               "-fPIC", "-shared", "-o", LIB, SRC, "-lhiprtc"])
    lib = C.CDLL(LIB)
    lib.rtx_hostemu_ray_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.rtx_hostemu_ray_table.restype = C.c_int64
    lib.rtx_hostemu_primary_dirs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtx_set_option.argtypes = [C.c_char_p, C.c_char_p]
    return lib


def _table(lib, sc, subimage=0, tasks=1):
    """(table [slots, 3] or None, primary_dir per pixel [H, ncols, 3]) of the scene's camera."""
    sd = sc.scene_desc()
    cd, _tables = sc.camera_desc(subimage, tasks)
    n = lib.rtx_hostemu_ray_table(C.addressof(sd), C.addressof(cd), None, 0)
    assert n >= 0
    tab = None
    if n:
        tab = np.zeros((n, 3), np.float32)
        assert lib.rtx_hostemu_ray_table(C.addressof(sd), C.addressof(cd), tab.ctypes.data, n) == n
    dirs = np.zeros((cd.height, cd.ncols, 3), np.float32)
    assert lib.rtx_hostemu_primary_dirs(C.addressof(sd), C.addressof(cd), dirs.ctypes.data) == 0
    return tab, dirs


def _slots(height, ncols):
    """The issue's layout, spelled out: slot of every (image row, strip column)."""
    r, cc = np.meshgrid(np.arange(height), np.arange(ncols), indexing="ij")
    tiles_x = (ncols + 7) >> 3
    return ((r >> 3) * tiles_x + (cc >> 3)) * 64 + (r & 7) * 8 + (cc & 7)


@pytest.mark.parametrize("res,strip", [((1, 1), (0, 1)), ((8, 8), (0, 1)), ((9, 7), (0, 1)), ((67, 45), (0, 1)),
                                       ((130, 9), (0, 1)), ((67, 45), (1, 2))])
def test_table_is_primary_dir_per_pixel(rays, res, strip):
    sc = product_scene_dict(U.tsp(res))
    tab, dirs = _table(rays, sc, *strip)
    H, W = dirs.shape[:2]
    assert tab is not None and len(tab) == ((H + 7) >> 3) * ((W + 7) >> 3) * 64  # ragged tiles whole
    s = _slots(H, W)
    assert len(np.unique(s)) == H * W and s.max() < len(tab)
    assert np.array_equal(tab[s].view(np.uint32), dirs.view(np.uint32))
    assert np.isfinite(tab).all()  # (the slots outside the image too)


def test_cameras_outside_the_class_have_no_table(rays):
    d = U.tsp((67, 45))
    d["AA"] = {"jitter": True, "samples": 1}
    assert _table(rays, product_scene_dict(d))[0] is None
    d["AA"] = {"jitter": False, "samples": 4}
    assert _table(rays, product_scene_dict(d))[0] is None
    assert _table(rays, product_scene("DepthOfField", (40, 24)))[0] is None
    assert _table(rays, product_scene("NovelScene1", (16, 12), AA={"jitter": False, "samples": 1}))[0] is None
    try:
        rays.rtx_set_option(b"ray_table", b"0")
        assert _table(rays, product_scene_dict(U.tsp((67, 45))))[0] is None
    finally:
        rays.rtx_set_option(b"ray_table", b"1")


@pytest.mark.parametrize("name,res", [("tsp", (9, 7)), ("tsp", (67, 45)), ("MirrorRefraction", (67, 45)),
                                      ("TorusMesh", (67, 45))])
def test_emulated_frames_equal_with_and_without_the_table(name, res, monkeypatch):
    d = U.tsp(res) if name == "tsp" else U.bundled(name, res)
    on, cnt_on = hostemu.render(product_scene_dict(d))
    monkeypatch.setattr(OPTS, "ray_table", "0")
    off, cnt_off = hostemu.render(product_scene_dict(d))
    assert on.astype(np.float32).tobytes() == off.astype(np.float32).tobytes()
    assert np.array_equal(cnt_on, cnt_off)
    rows = [3, 4, 5, 17, 18, 44] if res[1] > 44 else [1, 6]  # (rows off the tile grid)
    monkeypatch.setattr(OPTS, "ray_table", "1")
    part = hostemu.render_rows(product_scene_dict(d), rows)
    full = np.transpose(on, (1, 0, 2))[::-1].astype(np.float32)  # [row (0 = top), column, 3]
    assert part.tobytes() == np.ascontiguousarray(full[rows]).tobytes()


def _has_define(sc):
    spec = jit_spec(sc)
    return spec is not None and any(o.startswith("-DRTX_RAY_TABLE") for o in spec[1])


def test_jit_spec_carries_the_define_exactly_for_the_class(monkeypatch, tmp_path):
    one = {"AA": {"jitter": False, "samples": 1}}
    for name in ("TwoSpheresPlane", "TorusMesh"):
        spec = jit_spec(product_scene(name, (67, 45), **one))
        assert DEFINE in spec[1], name
    # secondary rays, and meshes without face boxes (more than 4096 faces: the corpus' 5,120-face
    # blob): measured slower with the table, so only on request (ray_table 4)
    d = meshgen.corpus_scene("blob4", meshgen.corpus(tmp_path))
    d["AA"] = {"jitter": False, "samples": 1}
    blob = product_scene_dict(d)
    for sc in (product_scene("MirrorRefraction", (67, 45), **one), blob):
        assert not _has_define(sc)
        monkeypatch.setattr(OPTS, "ray_table", "4")
        assert DEFINE in jit_spec(sc)[1]
        monkeypatch.setattr(OPTS, "ray_table", "1")
    assert not _has_define(product_scene("TwoSpheresPlane", (67, 45), AA={"jitter": True, "samples": 1}))
    assert not _has_define(product_scene("TwoSpheresPlane", (67, 45), AA={"jitter": False, "samples": 4}))
    assert not _has_define(product_scene("DepthOfField", (40, 24)))
    assert not _has_define(product_scene("MotionBlur", (40, 24)))
    monkeypatch.setattr(OPTS, "jit_ext", "1")  # (hierarchy kernels, specialized on request: no table)
    assert not _has_define(product_scene("NovelScene1", (16, 12), **one))
    monkeypatch.setattr(OPTS, "jit_ext", "0")
    sc = product_scene("TwoSpheresPlane", (130, 9), **one)  # 17 x 2 tiles x 768 B = 26112 B
    monkeypatch.setattr(OPTS, "ray_table_max_mb", "0.02")
    assert not _has_define(sc)
    monkeypatch.setattr(OPTS, "ray_table_max_mb", "0.025")
    assert _has_define(sc)
    monkeypatch.setattr(OPTS, "ray_table", "0")
    assert not _has_define(sc)


def test_default_cap_admits_1080p_and_2048x1024_not_4k(monkeypatch):
    one = {"AA": {"jitter": False, "samples": 1}}
    assert _has_define(product_scene("TwoSpheresPlane", (1920, 1080), **one))
    assert _has_define(product_scene("TwoSpheresPlane", (2048, 1024), **one))
    assert not _has_define(product_scene("TwoSpheresPlane", (3840, 2160), **one))
