"""The mesh corpus (tests/meshgen.py: open, planar, tied, degenerate, one-leaf, empty and
ill-scaled meshes; two and coincident top-level meshes) through every mesh path of
librtx.so on the MI355X: the scene-specialized and generic kernels, host- and device-built
face bins, heavy-tile chunks, light grids, the wave-cooperative variant, the first-hit
buffers, the ray entry points, sequence frames, row blocks and strips. Each path is held to
the oracle bit for bit (assert_parity) and the paths to each other (torch.equal).
tests/test_mesh_corpus.py runs the same scenes and rays through the host emulation and
asserts that they are not vacuous (coverage, hit rates, tie counts)."""
import copy

import numpy as np
import pytest
import torch

import meshgen
from common import OPTS, assert_parity, oracle_render_dict, product_scene_dict
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FLAT = [False, True]
MESH_KERNEL = "rtx_jit_render_1"  # rtx_jit_render_<mesh><sec><ext><count><jitter>


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return meshgen.corpus(tmp_path_factory.mktemp("corpus"))


_refs = {}


def oracle(name, corpus, flat, res=None):
    """The oracle's frame of a corpus scene, rendered once (read-only: shared by the tests)."""
    key = (name, flat, res)
    if key not in _refs:
        ref = oracle_render_dict(meshgen.corpus_scene(name, corpus, flat, res))
        assert not np.isnan(ref).any()
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def to_ref_layout(fb):
    """[rows, W, 3] (row 0 = top) -> the reference's float64 [column, row-from-bottom, rgb]."""
    return np.ascontiguousarray(np.transpose(fb.cpu().numpy()[::-1], (1, 0, 2))).astype(np.float64)


def frame_with(d, monkeypatch, **opts):
    """The frame of a fresh scene rendered under the given library options (they are read
    when the scene's camera and kernels are set up), and the kernel that rendered it."""
    with monkeypatch.context() as m:  # (the options' old values come back at its end)
        for k, v in opts.items():
            m.setattr(OPTS, k, v)
        sc = product_scene_dict(d)
        fb = sc.render_device().clone()
        return fb, sc.last_kernel


@pytest.mark.parametrize("flat", FLAT)
@pytest.mark.parametrize("name", list(meshgen.SCENES))
def test_default_render_matches_oracle(name, flat, corpus):
    d = meshgen.corpus_scene(name, corpus, flat)
    sc = product_scene_dict(d)
    img = sc.render()
    print(name, "flat" if flat else "smooth", "kernel", sc.last_kernel)
    # every corpus scene qualifies for a mesh-specialized kernel; the ones with a mirror or
    # glass run the secondary-ray form, the others the primary-and-shadow form
    sec = any(m.get("type", "diffuse") != "diffuse" for m in d["materials"])
    assert sc.last_kernel.startswith(MESH_KERNEL + ("1" if sec else "0")), sc.last_kernel
    assert sec == (name in ("two_mirror", "refractive"))
    assert_parity(img, oracle(name, corpus, flat), name)


@pytest.mark.parametrize("name", ["blob4", "dups", "head-on"])
def test_face_bins_and_heavy_tiles_equal_walk(name, corpus, monkeypatch):
    """One mesh: device-built face bins (two radix sorts) == host-built bins (stable_sort)
    == no bins (the BVH walk) == no heavy-tile pass == the oracle. blob4's bins are heavy at
    64 x 64; in `head-on` every face has one depth key, so the sorts must be stable alike."""
    d = meshgen.corpus_scene(name, corpus, flat=True)
    a, kernel = frame_with(d, monkeypatch)
    assert kernel.startswith(MESH_KERNEL), kernel
    assert_parity(to_ref_layout(a), oracle(name, corpus, True), name)
    for opts in (dict(dev_bins="0"), dict(bins="0"), dict(heavy_tiles="0"), dict(dev_bins="0", heavy_tiles="0")):
        b, kernel = frame_with(d, monkeypatch, **opts)
        assert torch.equal(a, b), (name, opts, kernel, float((a != b).float().mean()))


@pytest.mark.parametrize("name", ["blob3", "dups", "grid_bumpy", "below"])
def test_light_grids_equal_walk(name, corpus, monkeypatch):
    """The point lights' face grids == the BVH walk of the shadow rays == the oracle; two
    lights stand above the open surfaces and one below."""
    d = meshgen.corpus_scene(name, corpus, flat=False)
    a, kernel = frame_with(d, monkeypatch)
    b, _ = frame_with(d, monkeypatch, lgrid="0")
    assert torch.equal(a, b), (name, kernel)
    assert_parity(to_ref_layout(a), oracle(name, corpus, False), name)


@pytest.mark.parametrize("name", ["two", "two_mirror", "coincident", "empty", "dups"])
def test_generic_kernel_matches_oracle(name, corpus, monkeypatch):
    """The precompiled generic kernel (counts and the face-cull flag read at run time)."""
    d = meshgen.corpus_scene(name, corpus, flat=True)
    a, kernel = frame_with(d, monkeypatch, jit="0")
    assert kernel.startswith("k_render"), kernel
    assert_parity(to_ref_layout(a), oracle(name, corpus, True), name)


@pytest.mark.parametrize("name", ["dups", "head-on", "two", "two_mirror", "leaf9"])
def test_wave_cooperative_kernel_matches_oracle(name, corpus, monkeypatch):
    """-DRTX_WCOOP=1 with every mesh on it: its min-reduce applies the face-index tie rule
    (two_mirror: in the secondary-ray kernel, where only some of a wave's lanes reach a mesh)."""
    d = meshgen.corpus_scene(name, corpus, flat=True)
    a, kernel = frame_with(d, monkeypatch, jit_flags="-DRTX_WCOOP=1 -DRTX_WCOOP_MIN=1")
    assert kernel.startswith(MESH_KERNEL), kernel
    assert_parity(to_ref_layout(a), oracle(name, corpus, True), name)


@pytest.mark.parametrize("flat", FLAT)
@pytest.mark.parametrize("name", ["dups", "degenerate", "coincident", "head-on"])
def test_first_hit_buffers_match_oracle(name, flat, corpus):
    """render_aovs (k_aov): depth, normal, position, albedo, object and material ids of
    tied, degenerate and coincident faces against the oracle's closest hit."""
    from test_gpu_aov import run_case
    d = meshgen.corpus_scene(name, corpus, flat)
    _, got = run_case(d, name)
    mesh = 0 if name == "coincident" else 1
    assert float((got["object"] == mesh).mean()) >= 0.10
    assert not (got["object"] == 2).any()


def _gpu(sc):
    return (lambda o, d: sc.intersect(o, d, 0.0)), (lambda o, d, tmax: sc.occluded(o, d, tmax, 0.0))


@pytest.mark.parametrize("kind", meshgen.NONEMPTY)
def test_mesh_stress_rays_match_oracle(kind, corpus):
    """Scene.intersect / Scene.occluded on rays at the mesh's own vertices, edges and faces
    (meshgen.mesh_stress_rays) against the oracle, bit for bit, smooth and flat."""
    path = corpus[kind][0]
    o, dr = meshgen.mesh_stress_rays(*meshgen.read_obj(path), meshgen.N_RAYS, seed=1)
    for flat in FLAT:
        d = meshgen.one_mesh_scene(path, (8, 8), flat)
        meshgen.compare_rays(*_gpu(product_scene_dict(d)), O.OracleScene(copy.deepcopy(d), None), o, dr)


@pytest.mark.parametrize("how", ["big", "small", "far"])
@pytest.mark.parametrize("kind", ["blob3", "dups"])
def test_ill_scaled_stress_rays_match_oracle(kind, how, corpus):
    """The same rays around the mesh at scale 100, at scale 0.01 and 1000 units from the
    origin (the pads of the cluster and face boxes scale with |o| + cmax)."""
    path = corpus[kind][0]
    d = meshgen.conditioning_scene(path, how, flat=True)
    mesh = d["objects"][1]
    o, dr = meshgen.placed_rays(*meshgen.read_obj(path), meshgen.N_RAYS, 3, mesh["position"], mesh["scale"])
    meshgen.compare_rays(*_gpu(product_scene_dict(d)), O.OracleScene(copy.deepcopy(d), None), o, dr)


def test_coincident_meshes_stress_rays_match_oracle(corpus):
    path = corpus["grid_bumpy"][0]
    o, dr = meshgen.mesh_stress_rays(*meshgen.read_obj(path), meshgen.N_RAYS, seed=2)
    d = meshgen.coincident_scene(path, (8, 8))
    ob, _ = meshgen.compare_rays(*_gpu(product_scene_dict(d)), O.OracleScene(copy.deepcopy(d), None), o, dr, mesh=0)
    assert int((ob == 0).sum()) > 100 and not (ob == 2).any()


def test_sequence_frames_of_a_moving_mesh(corpus):
    """render_sequence with two windows on the moving mesh: each frame is the oracle's frame
    at that time, and what a render at that time gives."""
    d = meshgen.corpus_scene("moving", corpus)
    times = [0.0, 1.0]
    sc = product_scene_dict(d)
    fb = sc.render_sequence(times)
    assert sc.last_kernel.startswith(MESH_KERNEL), sc.last_kernel
    assert tuple(fb.shape) == (2, d["resolution"][1], d["resolution"][0], 3)
    assert not torch.equal(fb[0], fb[1])   # the ball moves (the reference's meshes ignore their speed)
    keep = list(sc.vc.motion_times)
    for f, t in enumerate(times):
        e = copy.deepcopy(d)
        e["motion"] = {"time": t, "samples": 0, "final": 1}   # the oracle's time table is [t]
        assert_parity(to_ref_layout(fb[f]), oracle_render_dict(e), "moving mesh t=%g" % t)
        sc.vc.motion_times = [t]
        assert torch.equal(sc.render_device(), fb[f]), f
    sc.vc.motion_times = keep


def test_row_blocks_and_strips_meet_ties(corpus):
    """`dups` at 43 x 29 (ragged 8 x 8 tiles): row blocks on and off the bins' 8-row grid
    equal the full frame's rows, and column strips equal the oracle's."""
    res = (43, 29)
    d = meshgen.corpus_scene("dups", corpus, flat=True, res=res)
    sc = product_scene_dict(d)
    full = sc.render_device().clone()
    assert_parity(to_ref_layout(full), oracle("dups", corpus, True, res), "dups 43x29")
    for row0, nrows in ((3, 13), (8, 21), (16, 13), (28, 1)):
        assert torch.equal(sc.render_device(row0=row0, nrows=nrows), full[row0:row0 + nrows]), (row0, nrows)
    for k in range(3):
        assert np.array_equal(sc.render(k, 3), oracle_render_dict(d, k, 3)), k
