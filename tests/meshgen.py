"""A corpus of small triangle meshes that the bundled torus and scenegen.blob_obj are not:
open, planar, with coincident and zero-area faces, of one BVH leaf, without faces -- and
the rays and scenes that put them before every mesh path. Plain Python, deterministic;
the OBJ files are written where the caller says (a test's tmp_path)."""
import copy

import numpy as np

from scenegen import blob_obj, blob_scene

KINDS = ("quad", "grid_planar", "grid_bumpy", "dups", "dups_planar", "degenerate", "leaf8", "leaf9", "empty",
         "blob3", "blob4")
NONEMPTY = tuple(k for k in KINDS if k != "empty")
N_RAYS = 8000  # stress rays per mesh, on the CPU and on the GPU (the same rays)


def _grid(n, bumpy, rng):
    """(n+1)^2 vertices on [-1, 1]^2 of the xz plane (y = 0, or random heights), 2 n^2
    triangles wound so that their normals point up (+y)."""
    xs = np.linspace(-1.0, 1.0, n + 1)
    V = np.array([[x, 0.0, z] for z in xs for x in xs])
    if bumpy:
        V[:, 1] = rng.uniform(-0.25, 0.25, len(V))
    F = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i          # (x0, z0)
            b, c, d = a + n + 1, a + 1, a + n + 2   # (x0, z1), (x1, z0), (x1, z1)
            F += [[a, b, c], [b, d, c]]
    return V, F


def read_obj(path):
    """Vertices (float64) and faces (int, 0-based) of a triangle OBJ file, as written."""
    V = [[float(x) for x in l.split()[1:4]] for l in open(path) if l.startswith("v ")]
    F = [[int(x) - 1 for x in l.split()[1:4]] for l in open(path) if l.startswith("f ")]
    return np.array(V, np.float64).reshape(-1, 3), np.array(F, np.int64).reshape(-1, 3)


def _write(path, V, F):
    with open(path, "w") as f:
        for v in V:
            f.write("v %.6f %.6f %.6f\n" % tuple(v))
        for a, b, c in F:
            f.write("f %d %d %d\n" % (a + 1, b + 1, c + 1))


def stress_mesh(kind, path, n=6, seed=0, swap_twins=False):
    """Write corpus mesh `kind` to `path`; returns (n_verts, n_faces, info).

    quad          2 faces in the plane y = 0: a zero-thickness bounding box
    grid_planar   n x n planar grid, 2 n^2 faces
    grid_bumpy    the same with random heights: an open surface
    dups          grid_bumpy, then every fifth face (0, 5, ...) once more, then faces 2, 7, ...
                  once more with reversed winding (the opposite flat normal). info["twins"]
                  maps the earlier face of each coincident pair to the later one,
                  info["flipped"] lists the earlier faces whose twin is the reversed one.
                  swap_twins: each flipped pair changes places in the file (the reversed copy
                  comes first), everything else equal
    dups_planar   dups on the planar grid
    degenerate    grid_bumpy with two zero-area faces in the middle of the face list (one
                  with a repeated index, one with two vertices at one position), on vertices
                  that no other face uses. info["degenerate"] lists their indices
    leaf8, leaf9  a 2 x 2 bumpy grid (8 faces: one BVH leaf), and the same with an upright
                  ninth face (the first split)
    empty         the 2 x 2 grid's vertices and no face
    blob3, blob4  scenegen.blob_obj levels 3 and 4 (1,280 and 5,120 closed faces)"""
    rng = np.random.RandomState(100 + seed)
    info = {}
    if kind in ("blob3", "blob4"):
        nv, nf = blob_obj(path, level=int(kind[4]), seed=seed)
        return nv, nf, info
    if kind == "quad":
        V, F = _grid(1, False, rng)
    elif kind == "grid_planar":
        V, F = _grid(n, False, rng)
    elif kind == "grid_bumpy":
        V, F = _grid(n, True, rng)
    elif kind in ("dups", "dups_planar"):
        V, F = _grid(n, kind == "dups", rng)
        nf = len(F)
        same, flip = list(range(0, nf, 5)), list(range(2, nf, 5))
        twins = {}
        F = [list(f) for f in F]
        for i in same:
            twins[i] = len(F)
            F.append(list(F[i]))
        for i in flip:
            twins[i] = len(F)
            a, b, c = F[i]
            F.append([a, c, b])
            if swap_twins:
                F[i], F[-1] = F[-1], F[i]
        info = {"twins": twins, "flipped": flip}
    elif kind == "degenerate":
        V, F = _grid(n, True, rng)
        k = len(V)
        # five vertices of their own, inside the grid's bounds; k+2 and k+3 share a position
        V = np.concatenate([V, [[0.3, 0.1, 0.2], [-0.4, 0.12, 0.5], [0.1, 0.05, -0.3], [0.1, 0.05, -0.3],
                                [0.6, 0.2, 0.6]]])
        h = len(F) // 2
        F = F[:h] + [[k, k + 1, k + 1], [k + 2, k + 3, k + 4]] + F[h:]
        info = {"degenerate": [h, h + 1]}
    elif kind in ("leaf8", "leaf9", "empty"):
        V, F = _grid(2, True, rng)
        if kind == "leaf9":
            k = len(V)
            V = np.concatenate([V, [[-0.5, 0.0, 0.1], [0.5, 0.0, -0.1], [0.0, 0.9, 0.0]]])
            F = F + [[k, k + 1, k + 2]]
        if kind == "empty":
            F = []
    else:
        raise ValueError(kind)
    _write(path, V, F)
    V, F = read_obj(path)
    if len(F):  # smooth normals stay finite on every vertex a face with area uses
        e = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
        live = np.linalg.norm(e, axis=1) > 0
        s = np.zeros_like(V)
        for k in range(3):
            np.add.at(s, F[live, k], e[live])
        used = np.unique(F[live])
        assert (np.linalg.norm(s[used], axis=1) > 1e-3).all(), kind
    return len(V), len(F), info


def mesh_stress_rays(V, F, n, seed=0, floor=-0.9):
    """Rays that stress a mesh's own geometry, in the style of scenegen.bv_stress_rays:
    aimed from both sides of the surface at every vertex, edge midpoint and face centroid
    (in turn, until there are n), from 0.5 to 30 units away. A quarter of the directions
    are rescaled by 10^U(-3, 3) (unnormalised shadow rays), an eighth of the origins lie
    on the mesh's bounding box and an eighth inside it, and an eighth of the directions
    have one or two exact zero components. floor: no ray starts below this height (the
    scenes' ground plane, at y = -1, would take those rays' closest hits); None: no floor.
    Returns float32 (n, 3) origins and directions."""
    rng = np.random.RandomState(seed)
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64)
    tri = V[F]
    cen = tri.mean(axis=1)
    # seven targets per face: its corners, its edges' midpoints, its centroid
    tgt = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2], (tri[:, 0] + tri[:, 1]) / 2, (tri[:, 1] + tri[:, 2]) / 2,
                          (tri[:, 2] + tri[:, 0]) / 2, cen])
    cen = np.tile(cen, (7, 1))
    pick = rng.permutation(len(tgt))[np.arange(n) % len(tgt)]
    tgt, cen = tgt[pick], cen[pick]
    # half of the rays aim at the point itself (on a border, rounding decides between hit
    # and miss), half a hair (1e-6 .. 1e-2 of the way to the centroid) inside the face
    s = np.where(rng.rand(n, 1) < 0.5, 0.0, 10.0 ** rng.uniform(-6, -2, (n, 1)))
    tgt = tgt + s * (cen - tgt)
    lo, hi = V.min(axis=0), V.max(axis=0)
    span = np.maximum(hi - lo, 0.0)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = np.where(rng.rand(n, 1) < 0.75, rng.uniform(0.5, 2.0, (n, 1)), rng.uniform(2.0, 30.0, (n, 1)))
    if floor is not None:  # rays that would start under the floor come from the other side
        d[(tgt - d * dist)[:, 1] < floor] *= -1.0
    o = tgt - d * dist
    kind = rng.randint(0, 8, n)
    # 0: origins on a face of the bounding box; 1: inside it
    box = lo + rng.uniform(0, 1, (n, 3)) * span
    ax = rng.randint(0, 3, n)
    side = rng.rand(n) < 0.5
    on = box.copy()
    on[np.arange(n), ax] = np.where(side, lo[ax], hi[ax])
    for k, src in ((0, on), (1, box)):
        m = kind == k
        o[m] = src[m]
        d[m] = tgt[m] - src[m]
    # 2: one or two exact zero components (the target's coordinates pass to the origin)
    m = kind == 2
    z = rng.rand(n, 3) < 0.45
    z[z.all(axis=1), 1] = False
    z[~z.any(axis=1), 0] = True
    dz = np.where(z, 0.0, d)
    if floor is not None:
        dz[(tgt - dz * dist)[:, 1] < floor] *= -1.0
    o[m] = (tgt - dz * dist)[m]
    d[m] = dz[m]
    # 3, 4: directions of very different magnitudes
    m = (kind == 3) | (kind == 4)
    d[m] *= 10.0 ** rng.uniform(-3, 3, (int(m.sum()), 1))
    bad = ~(np.abs(d).sum(axis=1) > 0)   # (an origin on its own target)
    d[bad] = [0.0, -1.0, 0.0]
    return o.astype(np.float32), d.astype(np.float32)


def placed_rays(V, F, n, seed, position=(0.0, 0.0, 0.0), scale=1.0):
    """mesh_stress_rays of the mesh as a scene places it: the reference's Mesh puts vertex v
    at (v + position) * scale, and so are the rays' origins; the directions stay."""
    o, d = mesh_stress_rays(V, F, n, seed)
    o = (o.astype(np.float64) + np.asarray(position, np.float64)) * scale
    return o.astype(np.float32), d


def compare_rays(intersect, occluded, osc, o, d, need_hits=0.5, mesh=1):
    """Closest hits (object, t, normal, position, material) and shadows (t_max 1 and inf)
    of rays o, d at time 0 against the oracle scene osc, bit for bit. intersect(o, d) and
    occluded(o, d, t_max) are the path under test (Scene.intersect / Scene.occluded or the
    host emulation's). At least need_hits of the rays hit object `mesh` by the oracle.
    Returns the oracle's (object, face) per ray."""
    got = intersect(o, d)
    t, ob, face, m, nn, pp = osc.closest(0.0, o, d)
    hit = ob >= 0
    rate = float((ob == mesh).mean())
    assert rate >= need_hits, rate
    assert not np.isnan(nn[hit]).any()
    assert np.array_equal(got["obj"], ob) and np.array_equal(got["mat"], m)
    assert np.array_equal(got["t"][hit], t[hit])
    assert np.array_equal(got["normal"][hit], nn[hit]) and np.array_equal(got["position"][hit], pp[hit])
    for tmax in (1.0, np.inf):
        assert np.array_equal(np.asarray(occluded(o, d, tmax)).astype(bool), osc.shadow(0.0, o, d, tmax).astype(bool))
    return ob, face


# ------------------------------------------------------------------------------ scenes
EXTRA_MATERIALS = [
    {"name": "mirror", "ID": 3, "type": "mirror", "diffuse": [0.2, 0.2, 0.25], "specular": [0.5, 0.5, 0.5],
     "hardness": 16, "tint": 0.3},
    {"name": "glass", "ID": 4, "type": "refractive", "diffuse": [0.1, 0.2, 0.1], "specular": [0.5, 0.5, 0.5],
     "hardness": 16, "tint": 0.3, "refr_index": 1.458},
    {"name": "blue", "ID": 5, "diffuse": [0.1, 0.2, 0.9], "specular": [0.3, 0.3, 0.3], "hardness": 8},
]


def one_mesh_scene(path, res=(64, 64), flat=False, view="above", material=2, **mesh_edits):
    """scenegen.blob_scene (the reference's TorusMesh scene: plane + mesh + three point
    lights) around one corpus mesh, with a nearer camera. view: "above" (from (0, 3, 3)),
    "below" (from under an open mesh, above the ground plane), "head-on" (straight down, up
    = -z: every face of a planar mesh at one depth) or "inside" (from inside the mesh's
    bounding volume, fov 100). mesh_edits go into the mesh's record (speed, scale ...)."""
    d = blob_scene(path, res, flat)
    # (a mirror or glass among the materials selects the secondary-ray kernels: only the
    # scenes that use one have it)
    d["materials"] = d["materials"] + [copy.deepcopy(m) for m in EXTRA_MATERIALS if m["ID"] in (5, material)]
    cam = d["camera"]
    if view == "above":
        cam["position"] = [0.0, 3.0, 3.0]
    elif view == "below":
        cam.update(position=[0.0, -0.8, 2.2], lookAt=[0.0, 0.0, 0.0])
    elif view == "head-on":
        cam.update(position=[0.0, 5.0, 0.0], up=[0.0, 0.0, -1.0])
    elif view == "inside":
        cam.update(position=[0.2, 0.1, 0.3], lookAt=[0.0, 0.0, -1.0], fov=100.0)
    else:
        raise ValueError(view)
    mesh = d["objects"][1]
    mesh["materials"] = [material]
    mesh.update(mesh_edits)
    return d


def two_mesh_scene(path_a, path_b, res=(64, 64), flat=False, mirror=False):
    """Two top-level meshes side by side (no face bins, no light grids; with one mesh of at
    most RTX_FACE_CULL_MAX faces and one above, the per-object face-cull mode). mirror:
    both meshes are mirrors, so secondary rays meet both."""
    d = one_mesh_scene(path_a, res, flat, material=3 if mirror else 2, position=[-1.0, 0.0, 0.0])
    d["camera"]["position"] = [0.0, 3.5, 3.5]
    other = copy.deepcopy(d["objects"][1])
    other.update(name="blob2", filepath=path_b, position=[1.0, 0.0, 0.0], materials=[3 if mirror else 5])
    d["objects"].append(other)
    return d


def coincident_scene(path, res=(64, 64), flat=False):
    """The same mesh twice at one place, clay first and blue second, with the ground plane
    between them in scene order: every hit ties across objects, and the first one wins."""
    d = one_mesh_scene(path, res, flat)
    plane, mesh = d["objects"]
    second = copy.deepcopy(mesh)
    second.update(name="second", materials=[5])
    d["objects"] = [mesh, plane, second]
    return d


def empty_scene(path, empty_path, res=(64, 64), flat=False):
    """one_mesh_scene plus a mesh without faces (its bounding box is in view)."""
    d = one_mesh_scene(path, res, flat)
    e = copy.deepcopy(d["objects"][1])
    e.update(name="empty", filepath=empty_path, position=[0.0, 0.5, 0.0], materials=[5])
    d["objects"].append(e)
    return d


def conditioning_scene(path, how, res=(64, 64), flat=False):
    """The one-mesh scene ill-scaled: how = "big" (scale 100, everything 100 times as far),
    "small" (scale 0.01, everything 100 times as near) or "far" (everything moved by
    [1000, 0, 1000])."""
    d = one_mesh_scene(path, res, flat)
    plane, mesh = d["objects"]
    if how in ("big", "small"):
        s = 100.0 if how == "big" else 0.01
        mesh["scale"] = s
        move = lambda p: [float(np.round(x * s, 6)) for x in p]  # noqa: E731
    elif how == "far":
        mesh["position"] = [1000.0, 0.0, 1000.0]
        move = lambda p: [p[0] + 1000.0, p[1], p[2] + 1000.0]  # noqa: E731
    else:
        raise ValueError(how)
    plane["position"] = move(plane["position"])
    d["camera"]["position"] = move(d["camera"]["position"])
    d["camera"]["lookAt"] = move(d["camera"]["lookAt"])
    if how == "small":
        # The reference starts a pixel's one AA sample 2 (dx + dy) image-plane units beside
        # the camera, in world x and y whatever the scene's size (its sunflower spread):
        # by (-0.038179, -0.034975) at 64 x 64, fov 45 -- more than this scene is wide. The
        # camera stands that much the other way, so the rays start where a camera at
        # (0, 0.03, 0.03) would put them (the tests' coverage bound holds the numbers).
        assert list(res) == [64, 64] and d["camera"]["fov"] == 45.0
        for key in ("position", "lookAt"):
            p = d["camera"][key]
            d["camera"][key] = [float(np.round(p[0] + 0.038179, 6)), float(np.round(p[1] + 0.034975, 6)), p[2]]
    for L in d["lights"]:
        L["position"] = move(L["position"])
    return d


def moving_scene(path, res=(43, 29), flat=False):
    """A top-level mesh with a `speed` under motion blur (3 shutter samples and the final
    time). The reference's Mesh never moves its vertices, so the mesh stays where it is -- but
    the scene is no longer static for the kernels, and a sphere that does move passes
    beside the mesh, so the frames differ and its shadow rays meet the mesh at every time."""
    d = one_mesh_scene(path, res, flat, speed=[0.5, 0.2, 0.0])
    d["objects"].append({"name": "ball", "type": "sphere", "radius": 0.3, "position": [-1.8, -0.6, 1.0],
                         "speed": [1.0, 0.0, 0.0], "materials": [5]})
    d["motion"] = {"time": 1.0, "samples": 3, "final": 1}
    return d


def corpus(dirpath):
    """Every corpus mesh written into dirpath: {kind: (path, n_verts, n_faces, info)}."""
    import os
    out = {}
    for kind in KINDS:
        p = os.path.join(str(dirpath), kind + ".obj")
        out[kind] = (p,) + stress_mesh(kind, p)
    return out


# scene name -> (builder(corpus, flat), {object index of a mesh: its least share of the pixels})
SCENES = {k: ((lambda c, flat, k=k: one_mesh_scene(c[k][0], flat=flat)), {1: 0.10})
          for k in NONEMPTY if k != "dups_planar"}
SCENES.update({
    "below": (lambda c, flat: one_mesh_scene(c["grid_bumpy"][0], flat=flat, view="below"), {1: 0.10}),
    "two": (lambda c, flat: two_mesh_scene(c["blob3"][0], c["blob4"][0], flat=flat), {1: 0.05, 2: 0.05}),
    "two_mirror": (lambda c, flat: two_mesh_scene(c["blob3"][0], c["blob4"][0], flat=flat, mirror=True),
                   {1: 0.05, 2: 0.05}),
    "coincident": (lambda c, flat: coincident_scene(c["grid_bumpy"][0], flat=flat), {0: 0.10}),
    "empty": (lambda c, flat: empty_scene(c["grid_bumpy"][0], c["empty"][0], flat=flat), {1: 0.10}),
    "head-on": (lambda c, flat: one_mesh_scene(c["dups_planar"][0], flat=flat, view="head-on"), {1: 0.10}),
    "big": (lambda c, flat: conditioning_scene(c["blob3"][0], "big", flat=flat), {1: 0.10}),
    "small": (lambda c, flat: conditioning_scene(c["blob3"][0], "small", flat=flat), {1: 0.10}),
    "far": (lambda c, flat: conditioning_scene(c["blob3"][0], "far", flat=flat), {1: 0.10}),
    "inside": (lambda c, flat: one_mesh_scene(c["blob3"][0], flat=flat, view="inside"), {1: 0.10}),
    "moving": (lambda c, flat: moving_scene(c["blob3"][0], flat=flat), {1: 0.10}),
    "refractive": (lambda c, flat: one_mesh_scene(c["blob3"][0], flat=flat, material=4), {1: 0.10}),
})
# the corpus kind whose twin faces a scene shows (its ties are between faces of one mesh)
TWINNED = {"dups": "dups", "head-on": "dups_planar"}


def corpus_scene(name, c, flat=False, res=None):
    d = SCENES[name][0](c, flat)
    if res is not None:
        d["resolution"] = list(res)
    return d


def first_hits(d, sc):
    """The oracle's closest hit of every pixel's first sample at the camera's first time,
    as (object, face) in image layout [H][W]; the rays are tests/test_gpu_aov.py's."""
    from oracle import oracle as O
    from test_gpu_aov import ASSETS, first_sample_rays, to_image
    o, dr = first_sample_rays(sc)
    W, H = o.shape[:2]
    _, ob, face, _, _, _ = O.OracleScene(copy.deepcopy(d), ASSETS).closest(float(sc.vc.motion_times[0]),
                                                                          o.reshape(-1, 3), dr.reshape(-1, 3))
    return to_image(ob.reshape(W, H)), to_image(face.reshape(W, H))


def check_first_wins(faces, info, all_hits=None):
    """faces: the oracle's winning face indices on one `dups` mesh. Returns how many lie on
    a coincident pair; every one of them must be the pair's earlier face. all_hits(i): every
    face of the mesh that ray i hits; with it a later twin may win where the ray misses the
    earlier one (a reversed twin tests its edges in another order, so on a border rounding
    can tell the two apart: no tie)."""
    faces = np.asarray(faces).ravel()
    later = np.isin(faces, list(info["twins"].values()))
    if all_hits is None:
        assert not later.any(), "the later twin won %d times" % int(later.sum())
    else:
        earlier = {b: a for a, b in info["twins"].items()}
        for i in np.nonzero(later)[0]:
            assert earlier[int(faces[i])] in info["flipped"] and earlier[int(faces[i])] not in all_hits(i), i
    return int(np.isin(faces, list(info["twins"])).sum())
