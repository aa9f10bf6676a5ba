"""Frame sequences on the MI355X (Scene.render_sequence / rtx_render_sequence): frame f of a
sequence is, bit for bit, what the existing path renders after ``vc.motion_times =
windows[f]`` -- and therefore the oracle's frame at those times -- for every kernel family
(scene-specialized and generic flat kernels, the mesh kernels, the hierarchy scenes' split
passes with their redo launch, the sample-parallel kernels), for row blocks, row groups and
sub-ranges of the sequence, with the culling structures (bins, shadow grids, light grids) on
and off, with lens sampling and Philox jitter, with counters, and from a captured graph.

References: a single-time frame at t is the C oracle with ``"motion": {"time": t, "samples":
0, "final": 1}`` (its time table is then exactly [t]); a window of several times is
oracle/pyloop.PyLoopScene with ``motion_times = window``. The bar is assert_parity
(frac_diff == 0), as everywhere in this suite.

Scene generator seeds (tests/scenegen.py; chosen on the CPU: at least one object has a
`speed`, and the oracle's first and last frames differ in the stated share of pixels at
43x29 over times 0 .. 2): random_scene 5 (mirror + refractive, AA 3; 8.0 %), shadow_scene 0
(two directional lights, three moving objects; 3.6 %), random_scene(mesh=True) 5 (14.9 %),
random_hier_scene 3 (three moving parts, AA 2; 14.3 %)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rtx
from common import OPTS, assert_parity, oracle_render_dict, product_scene_dict
from oracle import oracle as O
from rtx import _native as N
from rtx.io import ASSETS, bundled_scene_dict

pytestmark = pytest.mark.gpu

RES = (43, 29)  # odd: partial 8x8 tiles at the right and bottom edges, more than one block
TIMES = [0.0, 0.5, 1.0, 1.5, 2.0]


def to_ref_layout(fb):
    """[rows, W, 3] (row 0 = top) -> the reference's float64 [column, row-from-bottom, rgb]."""
    return np.ascontiguousarray(np.transpose(fb.cpu().numpy()[::-1], (1, 0, 2))).astype(np.float64)


def at_time(d, t):
    e = copy.deepcopy(d)
    e["motion"] = {"time": t, "samples": 0, "final": 1}
    return e


def motion_blur(res=RES, **edits):
    d = bundled_scene_dict("MotionBlur", resolution=res)
    d.pop("__base_dir__", None)
    d.update(edits)
    return d


@functools.lru_cache(maxsize=None)
def motion_blur_oracle(t):
    """The oracle's MotionBlur frame at the single time t (read-only: shared by the tests)."""
    ref = oracle_render_dict(at_time(motion_blur(), t))
    ref.setflags(write=False)
    return ref


def per_frame(sc, windows, **kw):
    """The renders the existing path offers: vc.motion_times = window, then render_device."""
    keep = list(sc.vc.motion_times)
    out = []
    for w in windows:
        sc.vc.motion_times = list(w) if np.ndim(w) else [w]
        out.append(sc.render_device(**kw).clone())
    sc.vc.motion_times = keep
    return out


@pytest.mark.parametrize("jit", ["1", "0"])
def test_motion_blur_single_time_frames(jit, monkeypatch):
    monkeypatch.setattr(OPTS, "jit", jit)
    sc = product_scene_dict(motion_blur())
    refs = [motion_blur_oracle(t) for t in TIMES]
    assert float((np.abs(refs[0] - refs[4]).max(axis=2) > 0).mean()) > 0.05  # the scene moves
    fb = sc.render_sequence(TIMES)
    assert sc.last_kernel.startswith("rtx_jit_render_") == (jit == "1"), sc.last_kernel
    u8 = sc.render_sequence(TIMES, rgb8=True)
    assert tuple(fb.shape) == (5, RES[1], RES[0], 3) and fb.dtype == torch.float32
    assert tuple(u8.shape) == (5, RES[1], RES[0], 3) and u8.dtype == torch.uint8
    for f, t in enumerate(TIMES):
        assert_parity(to_ref_layout(fb[f]), refs[f], "MotionBlur t=%g jit=%s" % (t, jit))
        assert np.array_equal(u8[f].cpu().numpy(), O.to_png_array(refs[f])), (f, jit)
    for f, want in enumerate(per_frame(sc, TIMES)):
        assert torch.equal(fb[f], want), (f, jit)
    for f, want in enumerate(per_frame(sc, TIMES, rgb8=True)):
        assert torch.equal(u8[f], want), (f, jit)
    assert not torch.equal(fb[0], fb[4])
    # batches of the sequence (one camera upload and launch each) give the same frames
    assert torch.equal(sc.render_sequence(TIMES, batch=2), fb)
    assert torch.equal(sc.render_sequence(TIMES, batch=1, rgb8=True), u8)


@pytest.mark.parametrize("jit", ["1", "0"])
def test_motion_blur_blurred_frames(jit, monkeypatch):
    """Windows of T = 3 times (2 shutter samples + the final one): the fp32 sums run in the
    reference's order and the divisor is samples * dof_samples * T."""
    from oracle import pyloop
    monkeypatch.setattr(OPTS, "jit", jit)
    d = motion_blur((24, 16))
    windows = rtx.frame_windows(0.0, 1.5, 3, shutter=0.4, samples=2, final=1)
    sc = product_scene_dict(d)
    fb = sc.render_sequence(windows)
    ps = pyloop.PyLoopScene(O.OracleScene(d, ASSETS))  # (its motion_times are assigned per window)
    for f, w in enumerate(windows):
        ps.motion_times = list(w)
        assert_parity(to_ref_layout(fb[f]), ps.render(), "MotionBlur window %d jit=%s" % (f, jit))
    for f, want in enumerate(per_frame(sc, windows)):
        assert torch.equal(fb[f], want), f


@pytest.mark.parametrize("jit", ["1", "0"])
def test_rows_groups_and_frame_ranges(jit, monkeypatch):
    monkeypatch.setattr(OPTS, "jit", jit)
    sc = product_scene_dict(motion_blur())
    W, H = RES
    windows = rtx.frame_windows(0.0, 2.0, 6)
    row0, nrows = 3, H // 2 - 1
    for dtype in (torch.float32, torch.uint8):
        rgb8 = dtype == torch.uint8
        out = torch.full((3, nrows + 4, W, 3), 7, dtype=dtype, device="cuda")
        sc.render_sequence(windows, out=out, row0=row0, nrows=nrows, frames=(2, 3))
        want = per_frame(sc, windows[2:5], row0=row0, nrows=nrows, rgb8=rgb8)
        for k in range(3):
            assert torch.equal(out[k, :nrows], want[k]), (dtype, k)
        assert bool((out[:, nrows:] == 7).all())
        want = per_frame(sc, windows[2:5], groups=(1, 3), rgb8=rgb8)
        g = want[0].shape[0]
        assert g == len(rtx.scene.group_rows(H, 3, 1))
        out = torch.full((3, g + 2, W, 3), 7, dtype=dtype, device="cuda")
        sc.render_sequence(windows, out=out, groups=(1, 3), frames=(2, 3))
        for k in range(3):
            assert torch.equal(out[k, :g], want[k]), (dtype, k)
        assert bool((out[:, g:] == 7).all())
    # the calls that know nothing of sequences render window 0 of a sequence camera
    sc.render_sequence(windows, frames=(5, 1))
    first = per_frame(sc, windows[:1])[0]
    sc.render_sequence(windows, frames=(5, 1))  # (the sequence camera again)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    N.call("rtx_render", sc._native.h, 0, H, C.c_void_p(a.data_ptr()), None, st)
    b = torch.empty((2, H, W, 3), dtype=torch.float32, device="cuda")
    N.call("rtx_render_frames", sc._native.h, 0, H, C.c_void_p(b.data_ptr()), 0, 2, H * W * 12, None, st)
    assert torch.equal(a, first) and torch.equal(b[0], first) and torch.equal(b[1], first)


def _family(d, times, what, oracle=True):
    """One sequence of single-time frames of scene d against the per-frame renders and the
    oracle; returns (scene, frames)."""
    sc = product_scene_dict(d)
    fb = sc.render_sequence(times)
    kern = sc.last_kernel
    refs = [oracle_render_dict(at_time(d, t)) for t in times] if oracle else []
    for f, ref in enumerate(refs):
        assert_parity(to_ref_layout(fb[f]), ref, "%s t=%g (%s)" % (what, times[f], kern))
    if refs:
        assert not np.array_equal(refs[0], refs[-1]), what
    for f, want in enumerate(per_frame(sc, times)):
        assert torch.equal(fb[f], want), (what, f, kern, sc.last_kernel)
    return sc, fb, kern


def _moving(objs):
    return sum(("speed" in o) + _moving(o.get("children", [])) for o in objs)


def _generated(gen, seed, **kw):
    import scenegen
    d = getattr(scenegen, gen)(seed, res=RES, **kw)
    d.pop("motion", None)
    assert _moving(d["objects"]) >= 1
    return d


@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("gen,seed,kw", [("random_scene", 5, {}), ("shadow_scene", 0, {}),
                                         ("random_scene", 5, {"mesh": True})])
def test_flat_kernel_families(gen, seed, kw, jit, monkeypatch):
    """Mirrors and refraction with moving objects, directional shadow grids, and the bins'
    object masks next to a mesh."""
    monkeypatch.setattr(OPTS, "jit", jit)
    d = _generated(gen, seed, **kw)
    sc, fb, kern = _family(d, [0.0, 1.0, 2.0], "%s %d %s" % (gen, seed, kw))
    assert kern.startswith("rtx_jit_render_") == (jit == "1"), kern


@pytest.mark.parametrize("jit", ["1", "0"])
def test_hierarchy_split_passes(jit, monkeypatch):
    """A moving hierarchy scene with AA 2: the three split passes and their redo launch
    (the precompiled ones, and those specialized on the scene's CSG trees); then with a
    record pool too small for the chains, so that the redo launch renders blocks."""
    monkeypatch.setattr(OPTS, "jit", jit)
    d = _generated("random_hier_scene", 3)
    d.pop("DOF", None)
    d["AA"] = {"jitter": False, "samples": 2}
    times = [0.0, 1.0, 2.0]
    sc, fb, kern = _family(d, times, "random_hier_scene 3")
    assert kern.startswith("rtx_jit_split_" if jit == "1" else "k_split_"), kern
    monkeypatch.setattr(OPTS, "split_ratio", "0")
    assert torch.equal(product_scene_dict(d).render_sequence(times), fb)


def test_hierarchy_sample_parallel_kernels(monkeypatch):
    """The same scene with spp_min lowered and the split passes off: the one-kernel
    sample-parallel form (render_body_spp)."""
    monkeypatch.setattr(OPTS, "spp_min", "2")
    monkeypatch.setattr(OPTS, "split", "0")
    d = _generated("random_hier_scene", 3)
    d.pop("DOF", None)
    d["AA"] = {"jitter": False, "samples": 2}
    sc, fb, kern = _family(d, [0.0, 1.0, 2.0], "random_hier_scene 3 spp")
    assert kern.endswith("_spp"), kern


def wide_scene():
    """A sphere and a box that cross the whole image over times -4 .. 4, in front of a static
    sphere and a torus mesh, under a directional and a point light."""
    mats = [{"name": "m%d" % i, "ID": i, "type": "diffuse", "diffuse": c, "specular": [0.5, 0.5, 0.5], "hardness": 16}
            for i, c in enumerate(([0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.3, 0.3, 0.9], [0.9, 0.9, 0.9]))]
    objs = [{"name": "ground", "type": "plane", "normal": [0.0, 1.0, 0.0], "position": [0.0, -1.0, 0.0],
             "materials": [3, 2]},
            {"name": "runner", "type": "sphere", "radius": 0.6, "position": [0.0, -0.2, 1.0], "materials": [0],
             "speed": [1.25, 0.0, 0.0]},
            {"name": "still", "type": "sphere", "radius": 0.8, "position": [-1.5, 0.0, -1.0], "materials": [1]},
            {"name": "slider", "type": "box", "position": [0.0, 1.4, 0.0], "size": [0.7, 0.5, 0.6], "materials": [2],
             "speed": [-1.0, 0.0, 0.25]},
            {"name": "torus", "type": "mesh", "filepath": "torus_mesh.obj", "scale": 0.8, "position": [1.5, -0.2, -0.5],
             "materials": [0], "flat_shaded": False}]
    lights = [{"name": "sun", "type": "directional", "direction": [0.4, -1.0, -0.3], "colour": [0.9, 0.9, 0.8],
               "power": 1.0},
              {"name": "lamp", "type": "point", "position": [-3.0, 4.0, 4.0], "colour": [0.6, 0.6, 0.9], "power": 0.8}]
    return {"resolution": list(RES), "AA": {"jitter": False, "samples": 1}, "ambient": [0.1, 0.1, 0.1],
            "camera": {"position": [0.0, 1.5, 8.0], "lookAt": [0.0, 0.2, 0.0], "up": [0.0, 1.0, 0.0], "fov": 50.0},
            "materials": mats, "objects": objs, "lights": lights}


def test_wide_time_range_and_culling_options(monkeypatch):
    """Over [-4, 4] the culling structures cover sweeps as wide as the image: the frames are
    exact with bins, dsgrid and lgrid on, and the same with each of them off (the generic
    kernels read the structures the host built, like the specialized ones)."""
    d = wide_scene()
    times = [-4.0, -2.0, 0.0, 2.0, 4.0]
    sc, fb, kern = _family(d, times, "wide range")
    assert kern.startswith("rtx_jit_render_1"), kern
    monkeypatch.setattr(OPTS, "jit", "0")
    assert torch.equal(product_scene_dict(d).render_sequence(times), fb)
    for opt in ("bins", "dsgrid", "lgrid"):
        monkeypatch.setattr(OPTS, opt, "0")
        assert torch.equal(product_scene_dict(d).render_sequence(times), fb), opt
        monkeypatch.setattr(OPTS, opt, "1")


def test_lens_samples_and_philox_jitter():
    """DOF 3 x AA 2 with the production (Philox) jitter: the jitter is keyed by pixel and
    sample, not by frame, so the frames equal the per-frame renders with the same seed."""
    d = motion_blur(AA={"jitter": True, "samples": 2}, DOF={"focal_length": 5.0, "aperture": 0.15, "samples": 3})
    sc = product_scene_dict(d)
    sc.seed = 1234
    windows = rtx.frame_windows(0.0, 2.0, 3, shutter=0.5, samples=2)
    fb = sc.render_sequence(windows)
    for f, want in enumerate(per_frame(sc, windows)):
        assert torch.equal(fb[f], want), (f, sc.last_kernel)
    assert not torch.equal(fb[0], fb[2])
    sc.seed = 1235
    assert not torch.equal(sc.render_sequence(windows), fb)


def test_counters_accumulate_over_the_frames():
    sc = product_scene_dict(motion_blur())
    times = TIMES[:3]
    total = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    fb = sc.render_sequence(times, counters=total)
    each = torch.zeros(N.RTX_COUNTERS, dtype=torch.int64, device="cuda")
    for f, want in enumerate(per_frame(sc, times, counters=each)):
        assert torch.equal(fb[f], want), f
    assert int(each[0]) == 3 * RES[0] * RES[1]  # one primary ray per pixel and frame
    assert torch.equal(total, each), (total.tolist(), each.tolist())


def test_ordinary_camera_after_a_sequence():
    """The sequence is part of the camera key: render() afterwards uploads the ordinary
    camera (the scene's own motion blur) and is exact; so is the sequence after it."""
    from common import oracle_render
    sc = product_scene_dict(motion_blur())
    fb = sc.render_sequence(TIMES[:2])
    ref = oracle_render("MotionBlur", RES)
    assert_parity(sc.render(), ref, "MotionBlur after a sequence")
    assert len(sc.vc.motion_times) > 1  # (a blurred frame: another sample count, other kernels)
    assert torch.equal(sc.render_sequence(TIMES[:2]), fb)
    assert_parity(to_ref_layout(fb[1]), motion_blur_oracle(TIMES[1]), "sequence again")


def test_frame_range_and_stride_errors():
    sc = product_scene_dict(motion_blur())
    W, H = RES
    sc.render_sequence(TIMES)
    buf = torch.empty((6, H, W, 3), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = C.c_void_p(buf.data_ptr())
    for fn, a, b in (("rtx_render_sequence", 0, H), ("rtx_render_groups_sequence", 0, 1)):
        N.call(fn, sc._native.h, a, b, p, 1, 3, 2, H * W * 3, None, st)        # frames [3, 5) of 5
        for frame0, n in ((3, 3), (5, 1), (0, 6)):                            # past the sequence
            with pytest.raises(N.RtxError, match="outside the camera's sequence") as e:
                N.call(fn, sc._native.h, a, b, p, 1, frame0, n, H * W * 3, None, st)
            assert e.value.code == N.RTX_ERR_INVALID
        with pytest.raises(N.RtxError, match="overlap") as e:                 # overlapping slots
            N.call(fn, sc._native.h, a, b, p, 1, 0, 2, H * W * 3 - 1, None, st)
        assert e.value.code == N.RTX_ERR_INVALID
        with pytest.raises(N.RtxError):
            N.call(fn, sc._native.h, a, b, p, 1, 0, 0, H * W * 3, None, st)    # no frames
    # a camera without a sequence holds one window
    sc.render_device()
    N.call("rtx_render_sequence", sc._native.h, 0, H, p, 1, 0, 1, H * W * 3, None, st)
    with pytest.raises(N.RtxError, match="outside the camera's sequence"):
        N.call("rtx_render_sequence", sc._native.h, 0, H, p, 1, 0, 2, H * W * 3, None, st)
    torch.cuda.synchronize()
    assert torch.equal(buf[0], sc.render_device(rgb8=True))


def test_sequence_launch_replays_from_a_graph():
    """One sequence launch of a flat scene recorded as a HIP graph (after an eager render,
    which uploads the camera and compiles the kernel) replays the same bytes."""
    sc = product_scene_dict(motion_blur())
    out = torch.zeros((5, RES[1], RES[0], 3), dtype=torch.uint8, device="cuda")
    sc.render_sequence(TIMES, out=out)
    assert sc.jit_wait() == 0
    torch.cuda.synchronize()
    want = out.clone()
    for f, t in enumerate(TIMES):
        assert np.array_equal(want[f].cpu().numpy(), O.to_png_array(motion_blur_oracle(t))), f
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        sc.render_sequence(TIMES, out=out)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
