"""Ranked id-coverage buffers (Scene.render_ids, rtx_render_ids) on the GPU, equal to the oracle
of tests/test_ids.py: Scene.camera_rays gives every sample ray, OracleScene.closest each ray's
object and material at each motion time (test_resolved.sample_hits), test_ids.rank the table and
the ranking. Philox jitter: the product draws on the device, the expectation comes from a second
Scene that replays oracle.philox.jitter_noise. Every comparison is np.array_equal (torch.equal on
the device); the samples of a case are computed once and shared. TwoSpheresPlane as bundled has
AA 3, so the comparison with render_aovs' first-sample buffers runs on a one-sample copy of it."""
import functools

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from common import OPTS, product_scene_dict
import test_ids as I
import test_resolved as R
import test_gpu_resolved as GR
from test_gpu_aov import bundle

pytestmark = pytest.mark.gpu

ALL = rtx.ID_NAMES
RES = GR.RES  # 50 x 37: ragged 8x8 tiles on both axes
KEYS = ("object", "material")
SENTINEL = -7


def host(buffers):
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in buffers.items()}


# ---------------------------------------------------------------- the cases and their expectations
def crowd(res=(40, 30)):
    """54 small spheres on a 9 x 6 grid in front of the DepthOfField bundle's plane, seen through
    a wide lens (32 DOF origins): pixels with many objects, ties, and more than eight keys."""
    d = bundle("DepthOfField", res, AA={"jitter": False, "samples": 1},
               DOF={"aperture": 0.8, "focal_length": 3.0, "samples": 32})
    objects = [d["objects"][0]]
    for iy in range(6):
        for ix in range(9):
            k = 9 * iy + ix
            objects.append({"type": "sphere", "name": "crowd%02d" % k, "radius": 0.13,
                            "position": [-1.2 + 0.3 * ix, 0.3 + 0.3 * iy, -1.5],
                            "materials": [d["materials"][k % 3]["ID"]]})
    d["objects"] = objects
    return d


def _blob(mesh_dir):
    return GR._blob(mesh_dir)


@pytest.fixture(scope="module")
def mesh_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ids_meshes"))


# name -> (scene dictionary from the mesh directory, replayed noise seed or None)
CASES = {n: GR.CASES[n] for n in ("tsp", "tsp_aa3_philox", "torus_aa2", "motionblur", "dof_replay", "dof_philox")}
CASES["tsp_one"] = (lambda _: GR._one_sample(bundle("TwoSpheresPlane", RES)), None)  # (the bundle has AA 3)
CASES["crowd"] = (lambda _: crowd(), None)
CASES["blob_aa2"] = (_blob, None)
SAMPLES = dict(tsp=3, tsp_one=1, tsp_aa3_philox=3, torus_aa2=2, motionblur=17, dof_replay=6, dof_philox=6, crowd=32, blob_aa2=2)


@functools.lru_cache(maxsize=None)
def case(name, mesh_dir=None):
    """(scene dictionary, the samples of test_resolved.sample_hits). Read-only for every test."""
    make, replay = CASES[name]
    d = make(mesh_dir)
    _, rays, _ = GR.scenes(d, replay)
    samples = R.sample_hits(d, rays, rays.vc.motion_times)
    for a in samples.values():
        a.setflags(write=False)
    assert R.is_flat(d) and samples["hit"].shape[0] == SAMPLES[name]
    return d, samples


def _keys(samples, key):
    return samples["obj" if key == "object" else "mat"]


@functools.lru_cache(maxsize=None)
def want(name, key, ranks, mesh_dir=None):
    _, samples = case(name, mesh_dir)
    ids, counts, other = I.rank(_keys(samples, key), samples["hit"], ranks)
    out = dict(ids=ids, counts=counts, other=other)
    for a in out.values():
        a.setflags(write=False)
    return out


def compare(got, exp, what, names=ALL):
    for n in names:
        assert got[n].dtype == np.int32 and got[n].shape == exp[n].shape, (what, n, got[n].shape, exp[n].shape)
        assert np.array_equal(got[n], exp[n]), (what, n, float((got[n] != exp[n]).mean()))


def check_alpha(sc, got, S, what, **kw):
    """fl32(sum(counts) + other) / fl32(S) is render_resolved's alpha, bit for bit."""
    alpha = host(sc.render_resolved(("alpha",), **kw))["alpha"]
    hits = got["counts"].sum(axis=-1, dtype=np.int32) + got["other"]
    assert np.array_equal(hits.astype(np.float32) / np.float32(S), alpha), what


# ---------------------------------------------------------------- scenes
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", ["tsp", "tsp_one", "tsp_aa3_philox", "torus_aa2", "motionblur", "dof_replay", "dof_philox"])
def test_scenes_match_the_oracle(name, key):
    d, samples = case(name)
    exp = want(name, key, 4)
    sc, _, _ = GR.scenes(d, CASES[name][1])
    H, W, S = sc.vc.height, sc.vc.width, sc.samples_per_pixel
    assert (W, H) == RES and S == SAMPLES[name]
    got = host(sc.render_ids(4, key))
    assert list(got) == list(ALL)
    compare(got, exp, (name, key))
    assert np.array_equal(got["counts"].sum(axis=-1) + got["other"], samples["hit"].sum(axis=0))
    assert (samples["hit"].any(axis=0)).mean() >= 0.05, (name, "hit pixels")
    check_alpha(sc, got, S, (name, key))
    if name == "tsp_one":  # one sample: rank 0 is the first-hit buffer, the other ranks are empty
        first = host(sc.render_aovs((key,)))[key]
        assert np.array_equal(got["ids"][..., 0], first)
        assert np.array_equal(got["counts"][..., 0], (first >= 0).astype(np.int32))
        assert (got["ids"][..., 1:] == -1).all() and not got["counts"][..., 1:].any() and not got["other"].any()
    if name == "tsp_aa3_philox":
        assert sc.jitter and sc.jitter_noise is None  # the last Philox pair is half used
    if name == "motionblur" and key == "object":
        assert R.mixed_share(samples) >= 0.10 and not exp["other"].any()
    if name.startswith("dof"):
        assert (I.distinct_keys(_keys(samples, key), samples["hit"]) >= 2).mean() >= 0.05


# ---------------------------------------------------------------- the crowd: overflow, ties, deep ranks
def test_the_crowd_case_is_not_vacuous():
    """On the oracle's values (measured with it: 16.7 %, 4.8 %, 15.4 %, 2 pixels of 1200; 68.8 %)."""
    d, samples = case("crowd")
    obj, hit = samples["obj"], samples["hit"]
    assert len(d["objects"]) == 55 and hit.shape == (32, 30, 40)
    n = I.distinct_keys(obj, hit)
    assert (n >= 3).mean() >= 0.10, (n >= 3).mean()
    exp = want("crowd", "object", 8)
    assert (exp["other"] > 0).mean() >= 0.02 and np.array_equal(exp["other"] > 0, n > 8)
    c = exp["counts"]
    assert ((c[..., :-1] == c[..., 1:]) & (c[..., 1:] > 0)).any(axis=-1).mean() >= 0.05
    # the first eight distinct keys are not the eight most frequent: a dropped key has more
    # samples than a kept one
    full = I.histogram(obj, hit, len(d["objects"]))
    kept = (exp["ids"][..., None, :] == np.arange(full.shape[-1])[:, None]).any(axis=-1)
    worst_kept = np.where(c > 0, c, 1 << 20).min(axis=-1)
    assert (np.where(kept, 0, full).max(axis=-1) > worst_kept).sum() >= 1
    nm = I.distinct_keys(samples["mat"], hit)
    assert (nm >= 2).mean() >= 0.10 and nm.max() == 3


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("ranks", [8, 4, 1])
def test_crowd(ranks, key):
    d, samples = case("crowd")
    exp = want("crowd", key, ranks)
    sc = product_scene_dict(d)
    assert sc.samples_per_pixel == 32
    got = host(sc.render_ids(ranks, key))
    assert got["ids"].shape == (30, 40, ranks)
    compare(got, exp, ("crowd", key, ranks))
    check_alpha(sc, got, 32, ("crowd", key, ranks))
    if key == "object":
        # where nothing is left over the ranks are the complete histogram: any matte is exact
        done = exp["other"] == 0
        everything = list(range(len(sc.objects)))
        ids, counts = sc.render_ids(ranks, key, ("ids", "counts")).values()
        alpha = sc.render_resolved(("alpha",))["alpha"]
        all_matte = rtx.id_matte(ids, counts, everything, 32)
        assert torch.equal(all_matte[torch.as_tensor(done).cuda()], alpha[torch.as_tensor(done).cuda()])
        if ranks == 8:
            assert 0.5 < done.mean() < 1.0
            row = [1 + 9 * 2 + ix for ix in range(9)]  # one row of the grid
            matte = sc.render_resolved(("matte",), matte=row)["matte"]
            mine = sc.id_matte(ids, counts, [sc.objects[i] for i in row])
            where = torch.as_tensor(done).cuda()
            assert torch.equal(mine[where], matte[where])
            share = (np.isin(samples["obj"], row) & samples["hit"]).sum(axis=0) / 32.0  # (the oracle's matte)
            assert R.partial_share(share[done]) >= 0.02, R.partial_share(share[done])  # (4.2 %: a soft matte)


# ---------------------------------------------------------------- heavy mesh tiles
@pytest.mark.parametrize("bins", ["1", "0"])
def test_heavy_mesh_tiles(bins, monkeypatch, mesh_dir):
    """The 81,920-face mesh at 64x48, AA 2: its tiles' face lists are heavy; with and without the bins."""
    d, samples = case("blob_aa2", mesh_dir)
    monkeypatch.setattr(OPTS, "bins", bins)  # (read when the camera is uploaded)
    sc = product_scene_dict(d)
    for key in KEYS:
        got = host(sc.render_ids(4, key))
        compare(got, want("blob_aa2", key, 4, mesh_dir), ("blob bins " + bins, key))
        check_alpha(sc, got, 2, ("blob bins " + bins, key))
    assert samples["hit"].shape == (2, 48, 64) and samples["hit"].any(axis=0).mean() >= 0.05


# ---------------------------------------------------------------- rows, strips, sequences
def test_row_blocks_and_strips():
    d, _ = case("dof_philox")
    exp = want("dof_philox", "object", 4)
    sc, _, _ = GR.scenes(d)
    W = sc.vc.width
    rows = host(sc.render_ids(row0=3, nrows=13))  # off the 8-row grid
    compare(rows, {n: exp[n][3:16] for n in exp}, "rows")
    col0, ncols = rtx.strip_columns(W, 1, 3)
    part = host(sc.render_ids(subimage=1, tasks=3))
    compare(part, {n: exp[n][:, col0:col0 + ncols] for n in exp}, "strip")
    check_alpha(sc, part, 6, "strip", subimage=1, tasks=3)
    empty = sc.render_ids(3, row0=5, nrows=0)
    assert empty["ids"].shape == (0, W, 3) == empty["counts"].shape and empty["other"].shape == (0, W)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in empty.values())
    # a strip's own expectation: its rays, its Philox counters
    sc, rays, _ = GR.scenes(d, subimage=1, tasks=3)
    s = R.sample_hits(d, rays, rays.vc.motion_times, subimage=1, tasks=3)
    for key in KEYS:
        ids, counts, other = I.rank(_keys(s, key), s["hit"], 4)
        compare(host(sc.render_ids(4, key, subimage=1, tasks=3)), dict(ids=ids, counts=counts, other=other),
                ("strip vs the oracle", key))


def test_sequence_frame():
    d = bundle("MotionBlur", RES)
    windows = rtx.frame_windows(0, 2, 3, shutter=0.5, samples=3)
    sc = product_scene_dict(d)
    got = host(sc.render_ids(4, windows=windows, frame=1))
    assert list(sc.vc.motion_times) == list(product_scene_dict(d).vc.motion_times)  # not touched
    s = R.sample_hits(d, sc, windows[1])
    assert s["hit"].shape[0] == 3
    ids, counts, other = I.rank(s["obj"], s["hit"], 4)
    compare(got, dict(ids=ids, counts=counts, other=other), "frame 1")
    check_alpha(sc, got, 3, "frame 1", windows=windows, frame=1)
    frame0 = host(sc.render_ids(4, windows=windows, frame=0))
    assert not np.array_equal(frame0["counts"], got["counts"])  # the scene moves
    with pytest.raises(ValueError):
        sc.render_ids(windows=windows, frame=3)


# ---------------------------------------------------------------- buffer selection
def test_selection_and_out_tensors():
    d, _ = case("dof_replay")
    sc, _, _ = GR.scenes(d, CASES["dof_replay"][1])
    H, W = sc.vc.height, sc.vc.width
    for ranks in (4, 3):  # (16-byte runs, and runs stored word by word)
        exp = want("dof_replay", "object", ranks)
        shape = lambda n: (H, W) if n == "other" else (H, W, ranks)  # noqa: E731
        fill = lambda n: torch.full(shape(n), SENTINEL, dtype=torch.int32, device="cuda")  # noqa: E731
        for n in ALL:  # every single buffer, into a sentinel-filled tensor of the caller's
            out = {n: fill(n)}
            got = sc.render_ids(ranks, "object", n, out=out)
            assert list(got) == [n] and got[n] is out[n]
            g = host(got)[n]
            assert not (g == SENTINEL).any(), n  # fully overwritten
            assert np.array_equal(g, exp[n]), (n, ranks)
        # a partial out: the other requested buffers are allocated; an unrequested one is untouched
        counts, spare = fill("counts"), fill("other")
        got = sc.render_ids(ranks, "object", ("ids", "counts"), out=dict(counts=counts))
        assert list(got) == ["ids", "counts"] and got["counts"] is counts
        compare(host(got), exp, "partial out", ("ids", "counts"))
        assert bool((spare == SENTINEL).all())
    with pytest.raises(ValueError):
        sc.render_ids(4, out=dict(other=torch.empty((W, H), dtype=torch.int32, device="cuda").t()))  # not contiguous
    with pytest.raises(ValueError):
        sc.render_ids(4, out=dict(other=torch.empty((H, W), dtype=torch.int64, device="cuda")))


def test_runs_at_every_rank_count_and_alignment():
    """Every ranks value against the oracle, through the raw call into a buffer that starts 4
    bytes past a 16-byte boundary as well: the runs are then stored word by word."""
    d, _ = case("motionblur")
    sc = product_scene_dict(d)
    H, W = sc.vc.height, sc.vc.width
    lib = N.load()
    for ranks in range(1, 9):
        exp = want("motionblur", "object", ranks)
        compare(host(sc.render_ids(ranks)), exp, ("ranks", ranks))
        n = H * W * ranks
        buf = torch.full((2 * n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        ids, counts = buf[1:1 + n], buf[n + 5:2 * n + 5]
        assert ids.data_ptr() % 16 == 4
        assert lib.rtx_render_ids(sc.native().h, 0, H, 0, N.RTX_ID_OBJECT, ranks, ids.data_ptr(), counts.data_ptr(), None,
                                  torch.cuda.current_stream().cuda_stream) == N.RTX_OK
        b = host(dict(b=buf))["b"]
        assert np.array_equal(b[1:1 + n].reshape(H, W, ranks), exp["ids"]), ranks
        assert np.array_equal(b[n + 5:2 * n + 5].reshape(H, W, ranks), exp["counts"]), ranks
        assert (b[:1] == SENTINEL).all() and (b[1 + n:n + 5] == SENTINEL).all() and (b[2 * n + 5:] == SENTINEL).all()


# ---------------------------------------------------------------- mattes out of the ranks
def test_id_matte_equals_the_resolved_matte():
    d, samples = case("motionblur")
    exp = want("motionblur", "object", 4)
    assert not exp["other"].any()  # (the oracle: three objects, every hit is in a written rank)
    sc = product_scene_dict(d)
    S = sc.samples_per_pixel
    b = sc.render_ids(4)
    moving = [1, 2]
    matte = sc.render_resolved(("alpha", "matte"), matte=moving)
    mine = rtx.id_matte(b["ids"], b["counts"], moving, S)
    assert mine.is_cuda and mine.dtype == torch.float32 and torch.equal(mine, matte["matte"])
    assert R.partial_share(host(dict(m=mine))["m"]) >= 0.05  # motion blur: a soft matte
    assert torch.equal(sc.id_matte(b["ids"], b["counts"], [sc.objects[2], 1]), matte["matte"])
    assert torch.equal(rtx.id_matte(b["ids"], b["counts"], [0, 1, 2], S), matte["alpha"])  # all objects: the coverage
    for i in range(3):
        one = sc.render_resolved(("matte",), matte=[i])["matte"]
        assert torch.equal(rtx.id_matte(b["ids"], b["counts"], [i], S), one), i
    # the same lookup on the host
    cpu = rtx.id_matte(b["ids"].cpu(), b["counts"].cpu(), moving, S)
    assert not cpu.is_cuda and torch.equal(cpu, matte["matte"].cpu())


# ---------------------------------------------------------------- refusals and the entry point's errors
def test_hierarchy_and_texture_scenes_are_refused():
    """The pass is built for flat scenes: the entry point says so and writes nothing."""
    for name in ("NovelScene1", "NovelScene2"):
        sc = product_scene_dict(bundle(name, (16, 8)))
        out = dict(ids=torch.full((8, 16, 4), SENTINEL, dtype=torch.int32, device="cuda"))
        with pytest.raises(N.RtxError, match="hierarchies or textures") as e:
            sc.render_ids(4, "object", ("ids",), out=out)
        assert e.value.code == N.RTX_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((out["ids"] == SENTINEL).all())


def test_entry_point_argument_errors():
    lib = N.load()
    sc = product_scene_dict(bundle("TwoSpheresPlane", (16, 8)))
    h = sc.native().h
    buf = torch.full((16 * 8 * 8,), SENTINEL, dtype=torch.int32, device="cuda")
    p = buf.data_ptr()

    def call(row0, nrows, frame, key=0, ranks=4, ids=p, counts=None, other=None):
        return lib.rtx_render_ids(h, row0, nrows, frame, key, ranks, ids, counts, other, None)
    assert call(0, 8, 0) == N.RTX_ERR_STATE
    assert b"rtx_render_ids: rtx_camera_set" in lib.rtx_last_error()
    sc.render_resolved(("alpha",))  # (uploads the camera)
    kernel = sc.last_kernel
    bad = [(0, 9, 0), (-1, 2, 0), (4, -1, 0), (7, 2, 0), (0, 8, 0, 0, 4, None), (0, 8, 1), (0, 8, -1), (0, 8, 0, 2),
           (0, 8, 0, -1), (0, 8, 0, 0, 0), (0, 8, 0, 1, 9), (0, 8, 0, 0, -4)]
    for args in bad:
        assert call(*args) == N.RTX_ERR_INVALID, args
        assert lib.rtx_last_error().startswith(b"rtx_render_ids: "), args
    assert call(0, 8, 0, 0, 4, None, None, None) == N.RTX_ERR_INVALID
    assert b"no buffer" in lib.rtx_last_error()
    assert call(0, 8, 0, 5) == N.RTX_ERR_INVALID and b"key 5" in lib.rtx_last_error()
    assert call(0, 8, 0, 0, 9) == N.RTX_ERR_INVALID and b"ranks 9" in lib.rtx_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())  # no refused call wrote anything
    assert call(8, 0, 0) == N.RTX_OK  # no rows: nothing to do
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert call(0, 8, 0, 1, 8, None, None, p) == N.RTX_OK  # one buffer is enough
    windows = rtx.frame_windows(0, 1, 2)
    sc.render_ids(windows=windows, frame=1)
    assert call(0, 8, 2) == N.RTX_ERR_INVALID
    assert b"frame 2" in lib.rtx_last_error()
    assert sc.last_kernel == kernel == ""  # rtx_last_kernel is left as it is
    torch.cuda.synchronize()
