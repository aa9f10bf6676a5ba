"""First-hit feature buffers (Scene.render_aovs, rtx_render_aov) on the GPU, bit for bit
against the oracle.

The rays are restated here in numpy fp32 (rtx.f32, GLM's operation order) from the
camera tables: the first sample of a pixel -- DOF origin 0, AA origin 0 (scene.py:54-61),
plus that sample's jitter draw (scene.py:63-65) -- at the camera's first motion time. They go to
OracleScene.closest, which gives depth, position, normal, object and material. The albedo
oracle is OracleScene.render of the scene lit flat (no lights, ambient 1, every material
diffuse, one sample): 0 + 1 * diffuse is exact and the clamp idle for diffuse <= 1, so that
frame is the reference's `diffuse` at the first hit, checkers, textures and hierarchy leaves
included. Every comparison is np.array_equal."""
import copy
import os

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from rtx import f32 as F
from common import OPTS, oracle_render_dict, product_scene_dict
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")
f32 = np.float32


def bundle(name, res, **edits):
    d, _ = O.load_bundle(name)
    d = copy.deepcopy(d)
    d["resolution"] = list(res)
    for k, v in edits.items():
        if k == "flat_shaded":
            for g in d["objects"]:
                if g["type"] == "mesh":
                    g["flat_shaded"] = v
        else:
            d[k] = v
    return d


def one_sample(d):
    """The scene seen through a one-sample camera: AA 1, no jitter, one DOF sample, time 0."""
    d = copy.deepcopy(d)
    d["AA"] = {"jitter": False, "samples": 1}
    if "DOF" in d:
        d["DOF"]["samples"] = 1
    d.pop("motion", None)
    return d


def is_one_sample(sc):
    return sc.samples == 1 and not sc.jitter and sc.vc.dof_samples == 1 and len(sc.vc.motion_times) == 1


def to_image(a):
    """[column][reference row (0 = bottom)] -> [image row (0 = top)][column]."""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1)[::-1])


def first_sample_rays(sc, subimage=0, tasks=1, noise=None):
    """Origins and directions [W][H][3] fp32 of the first sample of every pixel of the strip."""
    t = sc.camera_tables(subimage, tasks)
    vc = sc.vc
    u, v, w = (np.asarray(x, f32) for x in (vc.u, vc.v, vc.w))
    xs, ys = t["xs"].astype(f32), t["ys"].astype(f32)
    bdir = F.normalize((xs[:, None, None] * u + ys[None, :, None] * v) - w * f32(vc.d))   # scene.py:54
    focal = np.asarray(vc.position, f32) + bdir * f32(vc.focal_length)                      # scene.py:55
    d = F.normalize(focal - t["dof"][0].astype(f32))                                        # scene.py:58
    o = np.broadcast_to(t["aa"][0, 0].astype(f32), d.shape).copy()                          # scene.py:60-61
    if sc.jitter:                                                                           # scene.py:63-65
        nz = np.asarray(noise, np.float64).reshape(t["ncols"], vc.height, vc.dof_samples, sc.samples, 3)
        o = o + F.normalize(nz[:, :, 0, 0].astype(f32)) * f32(t["jscale"])
    return o.astype(f32), d.astype(f32)


def oracle_buffers(d, sc, time=None, subimage=0, tasks=1, noise=None, base=ASSETS):
    """The six buffers' expected values in image layout (albedo: see flat_lit)."""
    o, dr = first_sample_rays(sc, subimage, tasks, noise)
    W, H = o.shape[:2]
    time = float(sc.vc.motion_times[0]) if time is None else time
    t, ob, _, m, nn, pp = O.OracleScene(copy.deepcopy(d), base).closest(time, o.reshape(-1, 3), dr.reshape(-1, 3))
    img = lambda a: to_image(a.reshape((W, H) + a.shape[1:]))  # noqa: E731
    return dict(depth=img(t.astype(f32)), object=img(ob), material=img(m), normal=img(nn), position=img(pp))


def flat_lit(d, subimage=0, tasks=1, base=ASSETS):
    """The albedo oracle: the one-sample scene d lit flat, as float32 [H][W][3]."""
    d = copy.deepcopy(d)
    d["lights"] = []
    d["ambient"] = [1, 1, 1]
    for m in d["materials"]:
        m["type"] = "diffuse"
        assert all(0.0 <= float(x) <= 1.0 for x in m.get("diffuse", [0, 0, 0]))
    ref = O.OracleScene(d, base).render(subimage, tasks)
    return to_image(ref).astype(f32)


def host(buffers):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in buffers.items()}


def check(got, want, what, albedo=None, mat_diffuse=None):
    """got vs the oracle: ids everywhere, depth / normal / position on hit pixels, the miss
    values everywhere; albedo against the flat-lit render and / or the hit material's diffuse."""
    hit = want["object"] >= 0
    assert np.array_equal(got["object"], want["object"]), what
    assert np.array_equal(got["material"], want["material"]), what
    assert got["object"].dtype == np.int32 and got["material"].dtype == np.int32
    for n in ("depth", "normal", "position"):
        assert got[n].dtype == np.float32
        assert np.array_equal(got[n][hit], want[n][hit]), (what, n)
    miss = ~hit
    assert (got["object"][miss] == -1).all() and (got["material"][miss] == -1).all(), what
    assert np.isposinf(got["depth"][miss]).all() and np.isfinite(got["depth"][hit]).all(), what
    for n in ("normal", "position", "albedo"):
        assert (got[n][miss] == 0).all(), (what, n)
    if albedo is not None:
        assert np.array_equal(got["albedo"], albedo), (what, "albedo vs the flat-lit render")
    if mat_diffuse is not None:
        assert np.array_equal(got["albedo"][hit], mat_diffuse[want["material"][hit]]), (what, "albedo vs materials")
    return hit


def run_case(d, what, base=ASSETS, need_hits=True):
    sc = product_scene_dict(d)
    got = host(sc.render_aovs())
    H, W = sc.vc.height, sc.vc.width
    assert all(got[n].shape == ((H, W, 3) if n in ("normal", "position", "albedo") else (H, W)) for n in rtx.AOV_NAMES)
    want = oracle_buffers(d, sc, base=base)
    flat = not any(g["type"] == "node" or "texture" in g for g in d["objects"])
    diffuse = np.array([m.get("diffuse", [0, 0, 0]) for m in d["materials"]], np.float64).astype(f32) if flat else None
    hit = check(got, want, what, albedo=flat_lit(d, base=base) if is_one_sample(sc) else None, mat_diffuse=diffuse)
    if need_hits:
        assert 0.05 < hit.mean(), (what, hit.mean())
    return sc, got


FLAT = [("TwoSpheresPlane", {}), ("TwoSpheresPlane", {"AA": {"jitter": False, "samples": 1}}),
        ("MirrorRefraction", {}), ("TorusMesh", {}), ("TorusMesh", {"flat_shaded": True}),
        ("MotionBlur", {}), ("DepthOfField", {"AA": {"jitter": False, "samples": 2},
                                              "DOF": {"aperture": 0.2, "focal_length": 3.0, "samples": 3}})]


@pytest.mark.parametrize("name,edits", FLAT, ids=["%s%d" % (n, i) for i, (n, _) in enumerate(FLAT)])
def test_flat_scenes_match_the_oracle(name, edits):
    d = bundle(name, (50, 37), **edits)
    sc, _ = run_case(d, name)
    if name == "MotionBlur":
        assert len(sc.vc.motion_times) == 17
    if name == "DepthOfField":
        assert (sc.vc.dof_samples, sc.samples, sc.jitter) == (3, 2, False)


@pytest.mark.parametrize("seed", range(3))
def test_random_scenes_match_the_oracle(seed):
    from scenegen import random_scene
    run_case(random_scene(seed, res=(50, 37)), "random %d" % seed)
    run_case(one_sample(random_scene(seed, res=(50, 37))), "random %d, one sample" % seed)


def test_ties_follow_scene_order():
    from scenegen import tie_scene
    run_case(tie_scene(res=(50, 37)), "ties")


@pytest.mark.parametrize("name,res", [("NovelScene1", (96, 48)), ("NovelScene2", (64, 32))])
def test_novel_scenes_match_the_oracle(name, res):
    """Hierarchies and textures; the flat-lit render is the only texture oracle."""
    d = one_sample(bundle(name, res))
    sc, got = run_case(d, name)
    assert is_one_sample(sc)
    if name == "NovelScene1":  # its textured ground is in view: more colours than materials
        assert sc.objects[0].texture is not None
        assert len(np.unique(got["albedo"].reshape(-1, 3), axis=0)) > len(d["materials"])


@pytest.mark.parametrize("mesh", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_random_hierarchy_scenes_match_the_oracle(seed, mesh):
    from scenegen import random_hier_scene
    d = random_hier_scene(seed, mesh=mesh)
    run_case(d, "hier %d" % seed, need_hits=False)
    run_case(one_sample(d), "hier %d, one sample" % seed, need_hits=False)


def _dof_jitter():
    return bundle("DepthOfField", (40, 30), AA={"jitter": True, "samples": 2},
                  DOF={"aperture": 0.2, "focal_length": 3.0, "samples": 3})


def test_jitter_replay_matches_the_oracle():
    d = _dof_jitter()
    noise = np.random.RandomState(11).rand(40 * 30 * 3 * 2 * 3)
    sc = product_scene_dict(d)
    sc.jitter_noise = noise
    got = host(sc.render_aovs())
    hit = check(got, oracle_buffers(d, sc, noise=noise), "replay")
    assert hit.mean() > 0.05
    # the draw moves the origin: the unjittered rays give other positions
    plain = oracle_buffers(d, sc, noise=np.full(noise.shape, 0.5))
    assert not np.array_equal(plain["position"], got["position"])


def test_jitter_philox_matches_the_oracle():
    from oracle import philox as PH
    d = _dof_jitter()
    sc = product_scene_dict(d)
    assert sc.jitter and sc.jitter_noise is None
    got = host(sc.render_aovs())
    noise = PH.jitter_noise(sc.seed, 0, 40, 30, 3, 2)
    check(got, oracle_buffers(d, sc, noise=noise), "philox")
    # a strip draws with its columns' counters
    col0, ncols = rtx.strip_columns(40, 1, 3)
    part = host(sc.render_aovs(subimage=1, tasks=3))
    for n in rtx.AOV_NAMES:
        assert np.array_equal(part[n], got[n][:, col0:col0 + ncols]), n
    check(part, oracle_buffers(d, sc, subimage=1, tasks=3, noise=PH.jitter_noise(sc.seed, col0, ncols, 30, 3, 2)),
          "philox strip")


def _equal(a, b, what):
    for n in rtx.AOV_NAMES:
        assert np.array_equal(a[n], b[n], equal_nan=True), (what, n)


def test_row_blocks_and_strips_equal_the_full_pass():
    for d in (bundle("TorusMesh", (50, 37)), one_sample(bundle("NovelScene1", (50, 37)))):
        sc = product_scene_dict(d)
        full = host(sc.render_aovs())
        rows = host(sc.render_aovs(row0=3, nrows=21))   # off the 8-row grid of the bins
        _equal(rows, {n: full[n][3:24] for n in full}, "rows")
        rows = host(sc.render_aovs(row0=8, nrows=29))   # on it, ragged at the bottom
        _equal(rows, {n: full[n][8:37] for n in full}, "rows on the grid")
        col0, ncols = rtx.strip_columns(50, 1, 3)
        part = host(sc.render_aovs(subimage=1, tasks=3))
        _equal(part, {n: full[n][:, col0:col0 + ncols] for n in full}, "strip")
        assert host(sc.render_aovs(row0=5, nrows=0))["depth"].shape == (0, 50)


@pytest.mark.parametrize("lens", [False, True])
@pytest.mark.parametrize("seed", range(3))
def test_primary_bins_change_nothing(seed, lens, monkeypatch):
    from scenegen import bins_scene
    d = bins_scene(seed, lens=lens)
    on = host(product_scene_dict(d).render_aovs())
    monkeypatch.setattr(OPTS, "bins", "0")
    off = host(product_scene_dict(d).render_aovs())  # (the option is read when the camera is uploaded)
    monkeypatch.setattr(OPTS, "bins", "1")
    _equal(on, off, "bins seed %d" % seed)
    assert (on["object"] >= 0).any()


def test_heavy_mesh_tiles_walk_their_lists(tmp_path, monkeypatch):
    """The 81,920-face mesh at 64x64: its tiles' face lists are heavy (a render would read
    the chunk pass's results, which this pass does not have)."""
    from scenegen import blob_obj, blob_scene
    p = str(tmp_path / "blob6.obj")
    blob_obj(p, level=6)
    d = blob_scene(p, (64, 64))
    sc = product_scene_dict(d)
    on = host(sc.render_aovs())
    check(on, oracle_buffers(d, sc, base=str(tmp_path)), "blob", albedo=flat_lit(d, base=str(tmp_path)))
    monkeypatch.setattr(OPTS, "bins", "0")
    off = host(product_scene_dict(d).render_aovs())
    monkeypatch.setattr(OPTS, "bins", "1")
    _equal(on, off, "blob bins")
    assert (on["object"] == 1).sum() > 64  # the mesh fills more than one 8x8 tile (thousands of faces each)


def test_selection_and_out_tensors():
    sc = product_scene_dict(bundle("TwoSpheresPlane", (50, 37)))
    full = host(sc.render_aovs())
    depth = torch.full((37, 50), float("nan"), device="cuda")
    obj = torch.full((37, 50), -7, dtype=torch.int32, device="cuda")
    got = sc.render_aovs(("depth", "object"), out=dict(depth=depth, object=obj))
    assert sorted(got) == ["depth", "object"] and got["depth"] is depth and got["object"] is obj
    got = host(got)
    assert np.array_equal(got["depth"], full["depth"]) and np.array_equal(got["object"], full["object"])
    # a partial out: the other requested buffers are allocated
    alb = torch.full((37, 50, 3), float("nan"), device="cuda")
    got = sc.render_aovs(("material", "albedo"), out=dict(albedo=alb))
    assert list(got) == ["material", "albedo"] and got["albedo"] is alb
    got = host(got)
    assert np.array_equal(got["albedo"], full["albedo"]) and np.array_equal(got["material"], full["material"])
    one = host(sc.render_aovs("normal"))
    assert list(one) == ["normal"] and np.array_equal(one["normal"], full["normal"])
    with pytest.raises(ValueError):
        sc.render_aovs(("depth",), out=dict(depth=torch.empty((50, 37), device="cuda").t()))  # not contiguous
    with pytest.raises(ValueError):
        sc.render_aovs(("depth",), out=dict(depth=torch.empty((37, 50), dtype=torch.float64, device="cuda")))


def test_sequence_frames():
    d = bundle("MotionBlur", (50, 37))
    windows = rtx.frame_windows(0, 2, 3)
    sc = product_scene_dict(d)
    frames = [host(sc.render_aovs(windows=windows, frame=k)) for k in range(3)]
    assert list(sc.vc.motion_times) == list(product_scene_dict(d).vc.motion_times)  # not touched
    for k in range(3):
        other = product_scene_dict(d)
        other.vc.motion_times = windows[k]
        _equal(frames[k], host(other.render_aovs()), "frame %d" % k)
        check(frames[k], oracle_buffers(d, sc, time=windows[k][0]), "frame %d vs the oracle" % k)
    assert not np.array_equal(frames[0]["position"], frames[2]["position"])  # the scene moves
    with pytest.raises(ValueError):
        sc.render_aovs(windows=windows, frame=3)


def test_albedo_equals_the_flat_lit_image():
    d = bundle("TwoSpheresPlane", (50, 37), AA={"jitter": False, "samples": 1}, lights=[], ambient=[1, 1, 1])
    sc = product_scene_dict(d)
    img = sc.render_device().clone()
    alb = sc.render_aovs(("albedo",))["albedo"]
    assert torch.equal(img, alb)
    assert float(alb.max()) > 0.0


def test_pick():
    d = bundle("TwoSpheresPlane", (50, 37))
    sc = product_scene_dict(d)
    want = oracle_buffers(d, sc)
    seen = set()
    for row in range(0, 37, 4):
        for col in range(0, 50, 7):
            oi = int(want["object"][row, col])
            if oi in seen:
                continue
            seen.add(oi)
            p = sc.pick(col, row)
            if oi < 0:
                assert p["object"] is None and p["material"] is None and p["depth"] == float("inf")
                assert not p["normal"].any() and not p["position"].any() and not p["albedo"].any()
                continue
            assert p["object"] is sc.objects[oi] and p["material"] is sc.materials[int(want["material"][row, col])]
            assert p["depth"] == float(want["depth"][row, col])
            assert np.array_equal(p["position"], want["position"][row, col])
            assert np.array_equal(p["normal"], want["normal"][row, col])
            assert np.array_equal(p["albedo"], np.asarray(p["material"].diffuse, np.float32))
    assert len(seen - {-1}) >= 2


def test_entry_point_argument_errors():
    lib = N.load()
    sc = product_scene_dict(bundle("TwoSpheresPlane", (16, 8)))
    h = sc.native().h
    buf = torch.empty(16 * 8 * 3, device="cuda")
    p = buf.data_ptr()
    assert lib.rtx_render_aov(h, 0, 8, 0, p, None, None, None, None, None, None) == N.RTX_ERR_STATE
    assert b"rtx_render_aov: rtx_camera_set" in lib.rtx_last_error()
    sc.render_aovs(("depth",))
    kernel = sc.last_kernel
    for args in ((0, 9, 0, p), (-1, 2, 0, p), (4, -1, 0, p), (7, 2, 0, p), (0, 8, 0, None), (0, 8, 1, p),
                 (0, 8, -1, p)):
        row0, nrows, frame, ptr = args
        assert lib.rtx_render_aov(h, row0, nrows, frame, ptr, None, None, None, None, None, None) == N.RTX_ERR_INVALID
        assert lib.rtx_last_error().startswith(b"rtx_render_aov: "), args
    assert lib.rtx_render_aov(h, 8, 0, 0, p, None, None, None, None, None, None) == N.RTX_OK  # no rows: nothing to do
    windows = rtx.frame_windows(0, 1, 2)
    sc.render_aovs(("depth",), windows=windows, frame=1)
    assert lib.rtx_render_aov(h, 0, 8, 2, p, None, None, None, None, None, None) == N.RTX_ERR_INVALID
    assert b"frame 2" in lib.rtx_last_error()
    assert sc.last_kernel == kernel == ""  # rtx_last_kernel is left as it is
    torch.cuda.synchronize()
