"""The mesh corpus (tests/meshgen.py: open, planar, tied, degenerate, one-leaf, empty and
ill-scaled meshes) through the device source compiled for the host (tests/hostemu.py),
against the oracle, bit for bit. It shows that the corpus is within the oracle's reach and
that each case is not vacuous (the mesh is in view, the rays hit it, the ties occur and
the first face wins them); tests/test_gpu_mesh_corpus.py runs the same scenes and rays
through the kernels on the MI355X, and this file is its twin to debug on the CPU."""
import numpy as np
import pytest

import hostemu
import meshgen
from common import assert_parity, oracle_render_dict, product_scene_dict
from oracle import oracle as O

FLAT = [False, True]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return meshgen.corpus(tmp_path_factory.mktemp("corpus"))


def test_corpus_meshes_are_what_they_claim(corpus):
    sizes = {k: corpus[k][2] for k in meshgen.KINDS}
    assert sizes == dict(quad=2, grid_planar=72, grid_bumpy=72, dups=101, dups_planar=101, degenerate=74, leaf8=8,
                         leaf9=9, empty=0, blob3=1280, blob4=5120)
    for k in ("quad", "grid_planar", "dups_planar"):   # zero-thickness bounding boxes
        V, _ = meshgen.read_obj(corpus[k][0])
        assert V[:, 1].min() == V[:, 1].max() == 0.0
    for k in ("dups", "dups_planar"):
        V, F = meshgen.read_obj(corpus[k][0])
        info = corpus[k][3]
        assert len(info["twins"]) == 29 and len(info["flipped"]) == 14
        for a, b in info["twins"].items():
            assert a < b and sorted(F[a]) == sorted(F[b])
            same = any(np.array_equal(np.roll(F[a], s), F[b]) for s in range(3))
            assert same != (a in info["flipped"])
    V, F = meshgen.read_obj(corpus["degenerate"][0])
    area = np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    deg = corpus["degenerate"][3]["degenerate"]
    assert list(np.nonzero(area == 0)[0]) == deg and 0 < deg[0] and deg[1] < len(F) - 1
    assert len(set(F[deg[0]])) == 2 and len(set(F[deg[1]])) == 3
    others = np.delete(F, deg, axis=0)
    assert not np.isin(F[deg], others).any()   # their vertices are their own


@pytest.mark.parametrize("flat", FLAT)
@pytest.mark.parametrize("name", list(meshgen.SCENES))
def test_hostemu_corpus_scene(name, flat, corpus):
    """Bit-exact image and ray tallies; no NaN in the oracle's image; every mesh has its
    share of the pixels; ties between faces, or meshes, go to the first."""
    d = meshgen.corpus_scene(name, corpus, flat)
    sc = product_scene_dict(d)
    img, cnt = hostemu.render(sc)
    ref, tl = oracle_render_dict(d, tallies=True)
    assert not np.isnan(ref).any()
    s = assert_parity(img, ref, name)
    assert s["frac_diff"] == 0.0, s
    assert list(cnt[:10]) == tl[:10]
    ob, face = meshgen.first_hits(d, sc)
    for oi, least in meshgen.SCENES[name][1].items():
        share = float((ob == oi).mean())
        print(name, "object", oi, "share of the pixels %.3f" % share)
        assert share >= least, (name, oi, share)
    if name in meshgen.TWINNED:
        n = meshgen.check_first_wins(face[ob == 1], corpus[meshgen.TWINNED[name]][3])
        print(name, "pixels on a coincident pair of faces:", n)
        assert n > 100, n
    if name == "coincident":   # the second mesh (object 2) never wins
        assert int((ob == 0).sum()) > 100 and not (ob == 2).any()
    if name == "empty":
        assert not (ob == 2).any()


@pytest.mark.parametrize("name", list(meshgen.TWINNED))
def test_flipped_twins_show_in_the_shading(name, corpus, tmp_path):
    """With each reversed twin moved in front of its original in the file (nothing else
    changes) the oracle's flat-shaded image differs: the order of tied faces is visible."""
    kind = meshgen.TWINNED[name]
    p = str(tmp_path / "swapped.obj")
    meshgen.stress_mesh(kind, p, swap_twins=True)
    d = meshgen.corpus_scene(name, corpus, flat=True)
    e = meshgen.corpus_scene(name, {kind: (p,)}, flat=True)
    a, b = oracle_render_dict(d), oracle_render_dict(e)
    n = int((np.abs(a - b).max(axis=2) > 0).sum())
    print(name, "pixels that the twin order changes:", n)
    assert n >= 1
    # and the host emulation follows the swapped file too
    img, _ = hostemu.render(product_scene_dict(e))
    assert_parity(img, b, name + " swapped")


def test_hostemu_moving_scene_single_times(corpus):
    """The frames of the sequence test: the `moving` scene at times 0 and 1, each against
    the oracle; they differ (the ball moves; the mesh, whose speed the reference ignores,
    covers the same pixels)."""
    import copy
    d = meshgen.corpus_scene("moving", corpus)
    sc = product_scene_dict(d)
    refs, masks = [], []
    for t in (0.0, 1.0):
        e = copy.deepcopy(d)
        e["motion"] = {"time": t, "samples": 0, "final": 1}   # the oracle's time table is [t]
        refs.append(oracle_render_dict(e))
        sc.vc.motion_times = [t]
        img, _ = hostemu.render(sc)
        assert_parity(img, refs[-1], "moving t=%g" % t)
        masks.append(meshgen.first_hits(e, sc)[0] == 1)
    n = int((np.abs(refs[0] - refs[1]).max(axis=2) > 0).sum())
    print("moving: pixels that differ between t=0 and t=1:", n)
    assert n > 20 and np.array_equal(masks[0], masks[1]) and masks[0].mean() >= 0.10


def test_one_mesh_scenes_have_face_bins_and_light_grids(corpus):
    """The scenes whose bins and light grids the GPU tests switch off and on do have them:
    face lists in the primary-ray bins, and a grid for some light whose cells the shadow
    rays from the ground under the mesh fall into."""
    for name in ("blob4", "dups", "head-on"):
        sc = product_scene_dict(meshgen.corpus_scene(name, corpus, flat=True))
        got = hostemu.bins(sc)
        assert got is not None and got[1].max() > 0, name
        print(name, "bins with faces: %d of %d, the longest lists %d" % ((got[1] > 0).sum(), got[1].size, got[1].max()))
    p = np.array([[x, -1.0, z] for x in np.linspace(-0.8, 0.8, 9) for z in np.linspace(-0.8, 0.8, 9)], np.float32)
    for name in ("blob3", "dups", "grid_bumpy", "below"):
        sc = product_scene_dict(meshgen.corpus_scene(name, corpus))
        in_grid = 0
        for light in range(3):
            got = hostemu.occluded_light(sc, p, light, True)
            if got is not None:
                in_grid += int((got[1] >= 0).sum())
        print(name, "ground points in a light grid's cells:", in_grid)
        assert in_grid > 20, name


def test_blob4_bins_are_heavy(corpus):
    """blob4 at 64 x 64: some 8 x 8 bins list more faces than one chunk of the heavy-tile
    pass tests (kHeavyChunk = 16, rtx_api.hip)."""
    sc = product_scene_dict(meshgen.corpus_scene("blob4", corpus))
    _, nf = hostemu.bins(sc)
    heavy = int((nf > 16).sum())
    print("blob4 64x64: %d of %d bins are heavy, the longest lists %d faces" % (heavy, nf.size, nf.max()))
    assert heavy >= 4


def _emu(sc):
    return (lambda o, d: hostemu.intersect(sc, o, d, 0.0)), (lambda o, d, tmax: hostemu.occluded(sc, o, d, tmax, 0.0))


@pytest.mark.parametrize("kind", meshgen.NONEMPTY)
def test_hostemu_mesh_stress_rays(kind, corpus):
    """Rays at the mesh's own vertices, edges and faces (meshgen.mesh_stress_rays): closest
    hits and shadows against the oracle, bit for bit, flat and smooth."""
    path, _, _, info = corpus[kind]
    V, F = meshgen.read_obj(path)
    o, dr = meshgen.mesh_stress_rays(V, F, meshgen.N_RAYS, seed=1)
    assert (np.abs(dr) > 0).any(axis=1).all() and ((dr == 0).any(axis=1)).mean() > 0.05
    for flat in FLAT:
        d = meshgen.one_mesh_scene(path, (8, 8), flat)
        osc = O.OracleScene(d, None)
        ob, face = meshgen.compare_rays(*_emu(product_scene_dict(d)), osc, o, dr)
        if "twins" in info:
            idx = np.nonzero(ob == 1)[0]
            n = meshgen.check_first_wins(
                face[idx], info, lambda i: set(osc.object_intersect(1, 0.0, o[idx[i]], dr[idx[i]])[4].tolist()))
            print(kind, "flat" if flat else "smooth", "rays on a coincident pair of faces:", n)
            assert n > 100, n
    print(kind, "stress rays that hit the mesh: %.3f" % float((ob == 1).mean()))


@pytest.mark.parametrize("how", ["big", "small", "far"])
@pytest.mark.parametrize("kind", ["blob3", "dups"])
def test_hostemu_ill_scaled_stress_rays(kind, how, corpus):
    """The same rays around the mesh at scale 100, at scale 0.01 and 1000 units from the
    origin (the pads of the cluster and face boxes scale with |o| + cmax)."""
    path, _, _, info = corpus[kind]
    d = meshgen.conditioning_scene(path, how, flat=True)
    mesh = d["objects"][1]
    o, dr = meshgen.placed_rays(*meshgen.read_obj(path), meshgen.N_RAYS, 3, mesh["position"], mesh["scale"])
    ob, face = meshgen.compare_rays(*_emu(product_scene_dict(d)), O.OracleScene(d, None), o, dr)
    print(kind, how, "stress rays that hit the mesh: %.3f" % float((ob == 1).mean()))


def test_hostemu_coincident_meshes_stress_rays(corpus):
    """The rays at two coincident meshes: the first in scene order wins every tie."""
    path = corpus["grid_bumpy"][0]
    V, F = meshgen.read_obj(path)
    o, dr = meshgen.mesh_stress_rays(V, F, meshgen.N_RAYS, seed=2)
    d = meshgen.coincident_scene(path, (8, 8))
    ob, _ = meshgen.compare_rays(*_emu(product_scene_dict(d)), O.OracleScene(d, None), o, dr, mesh=0)
    assert int((ob == 0).sum()) > 100 and not (ob == 2).any()
