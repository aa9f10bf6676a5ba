"""Resolved buffers (Scene.render_resolved, rtx_render_resolved) on the GPU, bit for bit against
the oracle of tests/test_resolved.py: Scene.camera_rays gives every sample ray, OracleScene.closest
each ray's first hit at each motion time, numpy adds the samples in float32 in the contract's
order. Philox jitter: the product draws on the device, the expectation comes from a second Scene
that replays oracle.philox.jitter_noise. The albedo is also held against OracleScene.render of
the scene lit flat at the camera's full sampling, which does not pass through camera_rays.
Every comparison is np.array_equal; an expectation is computed once per case and shared."""
import copy
import functools

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from common import OPTS, product_scene_dict
from oracle import philox as PH
import test_resolved as R
from test_gpu_aov import bundle

pytestmark = pytest.mark.gpu

ALL = rtx.RESOLVED_NAMES
VEC = ("normal", "albedo")
RES = (50, 37)  # ragged 8x8 tiles on both axes


def host(buffers):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in buffers.items()}


# ---------------------------------------------------------------- the cases and their expectations
def _dof(jitter):
    return bundle("DepthOfField", RES, AA={"jitter": jitter, "samples": 2},
                  DOF={"aperture": 0.2, "focal_length": 3.0, "samples": 3})


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    """Where the cases that need a mesh file write it (once per module)."""
    return str(tmp_path_factory.mktemp("resolved_meshes"))


def _coincident(mesh_dir):
    import os
    import meshgen
    path = os.path.join(mesh_dir, "dups.obj")
    if not os.path.exists(path):
        meshgen.stress_mesh("dups", path)
    d = meshgen.coincident_scene(path, (43, 29))
    d["AA"] = {"jitter": False, "samples": 2}
    return d


def _blob(mesh_dir):
    import os
    from scenegen import blob_obj, blob_scene
    path = os.path.join(mesh_dir, "blob6.obj")
    if not os.path.exists(path):
        blob_obj(path, level=6)
    d = blob_scene(path, (64, 48))
    d["AA"] = {"jitter": False, "samples": 2}
    return d


# name -> (scene dictionary from the mesh directory, replayed noise seed or None)
CASES = {
    "tsp": (lambda _: bundle("TwoSpheresPlane", RES), None),
    "tsp_aa3_philox": (lambda _: bundle("TwoSpheresPlane", RES, AA={"jitter": True, "samples": 3}), None),
    "mirror": (lambda _: bundle("MirrorRefraction", RES), None),
    "torus_aa2": (lambda _: bundle("TorusMesh", RES, AA={"jitter": False, "samples": 2}), None),
    "motionblur": (lambda _: bundle("MotionBlur", RES), None),
    "dof": (lambda _: _dof(False), None),
    "dof_replay": (lambda _: _dof(True), 11),
    "dof_philox": (lambda _: _dof(True), None),
    "coincident_aa2": (_coincident, None),
    "blob_aa2": (_blob, None),
}


def scenes(d, replay=None, subimage=0, tasks=1):
    """(the product's scene, the scene that gives the rays, the noise table or None). The
    product draws Philox jitter itself; the rays then come from a second Scene replaying it."""
    sc = product_scene_dict(d)
    if not sc.jitter:
        return sc, sc, None
    H, (col0, ncols) = sc.vc.height, rtx.strip_columns(sc.vc.width, subimage, tasks)
    if replay is not None:
        noise = np.random.RandomState(replay).rand(ncols * H * sc.vc.dof_samples * sc.samples * 3)
        sc.jitter_noise = noise
        return sc, sc, noise
    noise = PH.jitter_noise(sc.seed, col0, ncols, H, sc.vc.dof_samples, sc.samples)
    rays = product_scene_dict(d)
    rays.jitter_noise = noise
    return sc, rays, noise


@functools.lru_cache(maxsize=None)
def case(name, mesh_dir):
    """``mesh_dir``: the module's mesh directory, for the cases that write a mesh file. (scene dictionary, expected buffers with the matte of ALL objects, the samples, the
    flat-lit albedo). Read-only for every test."""
    make, replay = CASES[name]
    d = make(mesh_dir)
    _, rays, noise = scenes(d, replay)
    everything = list(range(len(rays.objects)))
    want, samples = R.expected(d, rays, rays.vc.motion_times, R.ASSETS, matte=everything)
    flat = R.flat_lit(d, noise)
    for a in list(want.values()) + list(samples.values()) + [flat]:
        a.setflags(write=False)
    return d, want, samples, flat


def compare(got, want, what, names=None):
    for n in names if names is not None else [k for k in ALL if k in want and k in got]:
        assert got[n].dtype == np.float32 and got[n].shape == want[n].shape, (what, n)
        assert np.array_equal(got[n], want[n]), (what, n, float((got[n] != want[n]).mean()))


# ---------------------------------------------------------------- scenes
@pytest.mark.parametrize("name", [n for n in CASES if n != "blob_aa2"])
def test_scenes_match_the_oracle(name, mesh_dir):
    d, want, samples, flat = case(name, mesh_dir)
    sc, _, _ = scenes(d, CASES[name][1])
    everything = list(range(len(sc.objects)))
    got = host(sc.render_resolved(ALL, matte=everything))
    H, W = sc.vc.height, sc.vc.width
    assert all(got[n].shape == ((H, W, 3) if n in VEC else (H, W)) for n in ALL)
    S = sc.samples * sc.vc.dof_samples * len(sc.vc.motion_times)
    assert samples["hit"].shape == (S, H, W)
    assert (want["alpha"] > 0).mean() >= 0.05, (name, "hit pixels")
    compare(got, want, name, ("alpha", "matte", "depth", "normal") + (("albedo",) if "albedo" in want else ()))
    assert np.array_equal(got["albedo"], flat), (name, "albedo vs the flat-lit render")
    assert np.array_equal(got["matte"], got["alpha"])  # the matte of all objects is the coverage
    miss = want["alpha"] == 0
    assert np.isposinf(got["depth"][miss]).all() and np.isfinite(got["depth"][~miss]).all()
    assert not got["normal"][miss].any() and not got["albedo"][miss].any()
    # what keeps the case from being vacuous, on the oracle's values
    if name.startswith("dof"):
        assert (sc.vc.dof_samples, sc.samples) == (3, 2) and S == 6
        assert R.partial_share(want["alpha"]) >= 0.05, R.partial_share(want["alpha"])
        assert R.mixed_share(samples) >= 0.10, R.mixed_share(samples)
    if name == "motionblur":
        assert S == 17 and R.mixed_share(samples) >= 0.10, R.mixed_share(samples)
    if name == "tsp_aa3_philox":
        assert S == 3 and sc.jitter and sc.jitter_noise is None  # the last Philox pair is half used
    assert R.is_flat(d)


def test_the_first_sample_buffers_are_not_the_resolved_ones(mesh_dir):
    """Sensitivity: render_aovs' buffers, broadcast over the samples, differ from the expectation
    on the DepthOfField case -- the test can tell the two passes apart."""
    d, want, samples, _ = case("dof", mesh_dir)
    sc, _, _ = scenes(d)
    first = host(sc.render_aovs(("depth", "normal", "albedo", "object")))
    restated = dict(alpha=(first["object"] >= 0).astype(np.float32), depth=first["depth"], normal=first["normal"],
                    albedo=first["albedo"])
    for n in restated:
        assert not np.array_equal(restated[n], want[n]), n
    # and the first sample is the oracle's first sample
    assert np.array_equal(first["object"], samples["obj"][0])


@pytest.mark.parametrize("bins", ["1", "0"])
def test_heavy_mesh_tiles(bins, monkeypatch, mesh_dir):
    """The 81,920-face mesh at AA 2: its tiles' face lists are heavy; with and without the bins."""
    d, want, _, flat = case("blob_aa2", mesh_dir)
    monkeypatch.setattr(OPTS, "bins", bins)  # (read when the camera is uploaded)
    sc = product_scene_dict(d)
    got = host(sc.render_resolved(ALL, matte=[1]))
    compare(got, want, "blob bins " + bins, ("alpha", "depth", "normal", "albedo"))
    assert np.array_equal(got["albedo"], flat)
    assert (want["alpha"] > 0).mean() >= 0.05
    assert R.partial_share(got["matte"]) > 0 and (got["matte"] == 1).sum() > 64  # the mesh's edge, and whole tiles


# ---------------------------------------------------------------- rows, strips, sequences
def test_row_blocks_and_strips(mesh_dir):
    for name in ("dof_philox",):
        d, want, _, _ = case(name, mesh_dir)
        sc, _, _ = scenes(d)
        H, W = sc.vc.height, sc.vc.width
        full = host(sc.render_resolved())
        compare(full, want, name)
        rows = host(sc.render_resolved(row0=3, nrows=13))  # off the 8-row grid
        compare(rows, {n: want[n][3:16] for n in want}, name + " rows")
        col0, ncols = rtx.strip_columns(W, 1, 3)
        part = host(sc.render_resolved(subimage=1, tasks=3))
        compare(part, {n: want[n][:, col0:col0 + ncols] for n in want}, name + " strip")
        empty = sc.render_resolved(row0=5, nrows=0)
        assert empty["alpha"].shape == (0, W) and empty["normal"].shape == (0, W, 3)
    # a strip's own expectation: its rays, its Philox counters
    d = _dof(True)
    sc, rays, noise = scenes(d, subimage=1, tasks=3)
    want, _ = R.expected(d, rays, rays.vc.motion_times, subimage=1, tasks=3)
    got = host(sc.render_resolved(subimage=1, tasks=3))
    compare(got, want, "strip vs the oracle")
    assert np.array_equal(got["albedo"], R.flat_lit(d, noise, 1, 3))


def test_sequence_frame():
    d = bundle("MotionBlur", RES)
    windows = rtx.frame_windows(0, 2, 3, shutter=0.5, samples=3)
    sc = product_scene_dict(d)
    moving = [i for i, g in enumerate(d["objects"]) if "speed" in g]
    assert moving == [1, 2]
    got = host(sc.render_resolved(ALL, matte=moving, windows=windows, frame=1))
    assert list(sc.vc.motion_times) == list(product_scene_dict(d).vc.motion_times)  # not touched
    want, samples = R.expected(d, sc, windows[1], matte=moving)
    assert samples["hit"].shape[0] == 3
    compare(got, want, "frame 1")
    other = host(sc.render_resolved(ALL, matte=moving, windows=windows, frame=0))
    assert not np.array_equal(other["matte"], got["matte"])  # the scene moves
    with pytest.raises(ValueError):
        sc.render_resolved(windows=windows, frame=3)


# ---------------------------------------------------------------- buffer selection
def test_selection_and_out_tensors(mesh_dir):
    d, want, _, _ = case("dof", mesh_dir)
    sc, _, _ = scenes(d)
    H, W = sc.vc.height, sc.vc.width
    shape = lambda n: (H, W, 3) if n in VEC else (H, W)  # noqa: E731
    nan = lambda n: torch.full(shape(n), float("nan"), device="cuda")  # noqa: E731
    everything = list(range(len(sc.objects)))
    for n in ALL:  # every single buffer, into a NaN-filled tensor of the caller's
        out = {n: nan(n)}
        got = sc.render_resolved(n, matte=everything if n == "matte" else None, out=out)
        assert list(got) == [n] and got[n] is out[n]
        g = host(got)[n]
        assert not np.isnan(g).any(), n  # fully overwritten
        assert np.array_equal(g, want[n]), n
    # a partial out: the other requested buffers are allocated; an unrequested one is untouched
    alpha, spare = nan("alpha"), nan("depth")
    got = sc.render_resolved(("normal", "alpha"), out=dict(alpha=alpha))
    assert list(got) == ["normal", "alpha"] and got["alpha"] is alpha
    compare(host(got), want, "partial out", ("normal", "alpha"))
    assert bool(torch.isnan(spare).all())
    with pytest.raises(ValueError):
        sc.render_resolved(("alpha",), out=dict(alpha=torch.empty((W, H), device="cuda").t()))  # not contiguous
    with pytest.raises(ValueError):
        sc.render_resolved(("alpha",), out=dict(alpha=torch.empty((H, W), dtype=torch.float64, device="cuda")))


# ---------------------------------------------------------------- mattes
def test_mattes(mesh_dir):
    d, want, samples, _ = case("motionblur", mesh_dir)
    sc, _, _ = scenes(d)
    moving = [i for i, g in enumerate(d["objects"]) if "speed" in g]
    assert moving == [1, 2]
    resolve = lambda m: R.resolve(samples["hit"], samples["obj"], samples["depth"], samples["normal"],  # noqa: E731
                                  matte=m)["matte"]
    matte = lambda m: host(sc.render_resolved(("matte",), matte=m))["matte"]  # noqa: E731
    both = resolve(moving)
    assert R.partial_share(both) >= 0.05, R.partial_share(both)  # motion blur: soft mattes
    assert np.array_equal(matte(moving), both)                                      # a set
    assert np.array_equal(matte([1]), resolve([1]))                                 # one object
    assert np.array_equal(matte([sc.objects[2]]), resolve([2]))                     # given as the object
    assert np.array_equal(matte([2, 1, 1, sc.objects[2]]), both)                    # duplicates
    assert np.array_equal(matte([0, 1, 2]), want["alpha"])                          # all objects: the coverage
    assert np.array_equal(resolve([1]) + resolve([2]) + resolve([0]) > 0, want["alpha"] > 0)


def test_hierarchy_and_texture_scenes_are_refused():
    """The pass is built for flat scenes: the entry point says so and writes nothing."""
    for name in ("NovelScene1", "NovelScene2"):
        sc = product_scene_dict(bundle(name, (16, 8)))
        out = dict(alpha=torch.full((8, 16), float("nan"), device="cuda"))
        with pytest.raises(N.RtxError, match="hierarchies or textures") as e:
            sc.render_resolved(("alpha",), out=out)
        assert e.value.code == N.RTX_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool(torch.isnan(out["alpha"]).all())


# ---------------------------------------------------------------- one-sample cameras, the colour
def _one_sample(d):
    d = copy.deepcopy(d)
    d["AA"] = {"jitter": False, "samples": 1}
    if "DOF" in d:
        d["DOF"]["samples"] = 1
    d.pop("motion", None)
    return d


@pytest.mark.parametrize("name,res", [("TwoSpheresPlane", RES), ("TorusMesh", RES)])
def test_one_sample_cameras_equal_the_first_hit_buffers(name, res):
    sc = product_scene_dict(_one_sample(bundle(name, res)))
    assert sc.samples * sc.vc.dof_samples * len(sc.vc.motion_times) == 1 and not sc.jitter
    first = host(sc.render_aovs(("depth", "normal", "albedo", "object")))
    got = host(sc.render_resolved(ALL, matte=[0]))
    assert np.array_equal(got["alpha"], (first["object"] >= 0).astype(np.float32))
    assert np.array_equal(got["matte"], (first["object"] == 0).astype(np.float32))
    for n in ("depth", "normal", "albedo"):
        assert np.array_equal(got[n], first[n]), n  # as values: -0 == +0
    assert not np.signbit(got["normal"][got["normal"] == 0]).any()  # a -0 component is +0 after the sum
    assert (first["object"] >= 0).mean() >= 0.05


def test_albedo_equals_the_flat_lit_colour(monkeypatch):
    """Against the colour: on a flat-lit scene, albedo is render_device's frame at full sampling
    (through the generic render kernel: no compile of a specialized one)."""
    monkeypatch.setattr(OPTS, "jit", "0")
    for d in (_dof(True), bundle("MotionBlur", RES)):
        d = copy.deepcopy(d)
        d["lights"], d["ambient"] = [], [1, 1, 1]
        for m in d["materials"]:
            m["type"] = "diffuse"
        sc = product_scene_dict(d)
        img = sc.render_device().clone()
        alb = sc.render_resolved(("albedo",))["albedo"]
        assert torch.equal(img, alb)
        assert 0.0 < float(alb.max()) <= 1.0


def test_rgba_image(monkeypatch):
    """The CLI's --rgba frame: the PNG bytes of the colour, and rtx_fb_to_rgb8 of alpha as A."""
    from rtx import main as cli
    monkeypatch.setattr(OPTS, "jit", "0")  # (no compile of a specialized render kernel)
    sc = product_scene_dict(_dof(False))
    rgb = sc.render_rgb8()
    img = cli.rgba_image(rgb, sc)
    alpha = host(sc.render_resolved(("alpha",)))["alpha"]
    assert img.dtype == np.uint8 and img.shape == rgb.shape[:2] + (4,)
    assert np.array_equal(img[..., :3], rgb)
    assert np.array_equal(img[..., 3], (alpha.astype(np.float64) * 255.0).astype(np.uint8))
    assert len(np.unique(img[..., 3])) > 2  # partial coverage reaches the file


# ---------------------------------------------------------------- the entry point's errors
def test_entry_point_argument_errors():
    lib = N.load()
    sc = product_scene_dict(bundle("TwoSpheresPlane", (16, 8)))
    h = sc.native().h
    buf = torch.full((16 * 8 * 3,), float("nan"), device="cuda")
    p = buf.data_ptr()
    ids = (N.C.c_int32 * 3)(0, 2, 2)

    def call(row0, nrows, frame, alpha, matte=None, objs=None, n=0):
        return lib.rtx_render_resolved(h, row0, nrows, frame, alpha, matte, None, None, None, objs, n, None)
    assert call(0, 8, 0, p) == N.RTX_ERR_STATE
    assert b"rtx_render_resolved: rtx_camera_set" in lib.rtx_last_error()
    sc.render_resolved(("alpha",))
    kernel = sc.last_kernel
    n_obj = len(sc.objects)
    bad = [(0, 9, 0, p), (-1, 2, 0, p), (4, -1, 0, p), (7, 2, 0, p), (0, 8, 0, None), (0, 8, 1, p), (0, 8, -1, p),
           (0, 8, 0, None, p, None, 1), (0, 8, 0, None, p, ids, 0), (0, 8, 0, None, p, ids, -2),
           (0, 8, 0, p, p, (N.C.c_int32 * 2)(0, n_obj), 2), (0, 8, 0, p, p, (N.C.c_int32 * 1)(-1), 1),
           (0, 8, 0, p, p, (N.C.c_int32 * 1)(N.RTX_MATTE_MAX_OBJECTS), 1)]
    for args in bad:
        assert call(*args) == N.RTX_ERR_INVALID, args[:3]
        assert lib.rtx_last_error().startswith(b"rtx_render_resolved: "), args[:3]
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())  # no refused call wrote anything
    assert call(8, 0, 0, p) == N.RTX_OK  # no rows: nothing to do
    # the matte arguments are ignored without the matte buffer
    assert call(0, 8, 0, p, None, None, -5) == N.RTX_OK
    assert call(0, 8, 0, None, p, ids, 3) == N.RTX_OK
    windows = rtx.frame_windows(0, 1, 2)
    sc.render_resolved(("alpha",), windows=windows, frame=1)
    assert call(0, 8, 2, p) == N.RTX_ERR_INVALID
    assert b"frame 2" in lib.rtx_last_error()
    assert sc.last_kernel == kernel == ""  # rtx_last_kernel is left as it is
    torch.cuda.synchronize()
