"""Tests-only: what Scene.render_light_groups must return, from the oracle alone. Plane g of a
case is OracleScene's render of the scene description edited to hold only group g's lights (in
their order) and a zero ambient unless g is the ambient's group -- the contract of
rtx_render_light_groups word for word, so no part of the pass is restated here."""
import copy
import functools
import os

import numpy as np

import rtx
from oracle import oracle as O
from oracle import philox as PH
from test_gpu_aov import bundle

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")
f32 = np.float32
RES = (50, 37)  # ragged 8x8 tiles on both axes


def edited(d, lights, ambient_on):
    """The scene dictionary with only the lights ``lights`` (indices, kept in their order) and
    with the ambient zeroed unless ``ambient_on``."""
    e = copy.deepcopy(d)
    e["lights"] = [copy.deepcopy(d.get("lights", [])[li]) for li in sorted(lights)]
    if not ambient_on:
        e["ambient"] = [0, 0, 0]
    return e


def to_rows(ref):
    """An oracle image [column][row from the bottom] as the framebuffer's float32 [row][column]."""
    return np.ascontiguousarray(np.swapaxes(ref, 0, 1)[::-1]).astype(f32)


def expected(d, groups, ambient, noise=None, subimage=0, tasks=1):
    """float32 [G][H][W][3], read-only: one oracle render per group of
    rtx.light_group_table(len(lights), groups, ambient)."""
    table, n_groups, ambient_group = rtx.light_group_table(len(d.get("lights", [])), groups, ambient)
    planes = []
    for g in range(n_groups):
        e = edited(d, [li for li in range(len(table)) if table[li] == g], ambient_group == g)
        planes.append(to_rows(O.OracleScene(e, ASSETS).render(subimage, tasks, noise=noise)))
    out = np.stack(planes)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- the cases
def _with_light(d, light):
    d = copy.deepcopy(d)
    d["lights"] = list(d["lights"]) + [light]
    return d


def _point(position, power, colour=(1.0, 1.0, 1.0)):
    return dict(name="extra", type="point", position=[float(x) for x in position], power=float(power),
                colour=[float(x) for x in colour])


def _mirror2():
    d = bundle("MirrorRefraction", RES)
    p = d["camera"]["position"]
    return _with_light(d, _point([p[0], p[1] + 2.0, p[2]], 0.8))  # the camera's position raised by 2


def _motionblur2():
    d = bundle("MotionBlur", RES)
    return _with_light(d, dict(name="extra", type="directional", direction=[1.0, -1.0, -1.0], power=0.6,
                               colour=[1.0, 1.0, 1.0]))


def _dof2():
    d = bundle("DepthOfField", RES, AA={"jitter": True, "samples": 2},
               DOF={"aperture": 0.2, "focal_length": 3.0, "samples": 3})
    return _with_light(d, _point([-2.0, 4.0, 3.0], 0.8))


def _nolights():
    d = bundle("TwoSpheresPlane", RES)
    d["lights"] = []
    return d


# name -> (scene dictionary, groups, ambient, jitter: None | "philox" | a replay seed)
CASES = {
    "tsp": (lambda: bundle("TwoSpheresPlane", RES), [[0], [1]], "own", None),
    "mirror2": (_mirror2, [[0], [1]], 0, None),
    "torus": (lambda: bundle("TorusMesh", RES), [[0], [1, 2]], None, None),
    "motionblur2": (_motionblur2, [[0], [1]], 1, None),
    "dof_replay": (_dof2, [[0], [1]], "own", 11),
    "dof_philox": (_dof2, [[0], [1]], "own", "philox"),
    "excluded": (lambda: bundle("TwoSpheresPlane", RES), [[0]], 0, None),
    "nolights": (_nolights, [[]], 0, None),
}


def noise_for(d, jitter, subimage=0, tasks=1):
    """The jitter draws of the case's camera as the oracle replays them, or None: a seeded
    np.random stream (the product replays it too), or the product's own Philox draws."""
    if jitter is None:
        return None
    sc = rtx.load_scene(dict(copy.deepcopy(d), __base_dir__=ASSETS), verbose=False)
    H, (col0, ncols) = sc.vc.height, rtx.strip_columns(sc.vc.width, subimage, tasks)
    if jitter == "philox":
        return PH.jitter_noise(sc.seed, col0, ncols, H, sc.vc.dof_samples, sc.samples)
    return np.random.RandomState(jitter).rand(ncols * H * sc.vc.dof_samples * sc.samples * 3)


def check_planes(name, table, n_groups, ambient_group, planes):
    """What keeps a case from passing with a black or a swapped plane, on the oracle's values:
    every group that holds a light or the ambient is non-zero in more than 5 % of its pixels,
    and any two planes differ in more than 5 % of them."""
    for g in range(n_groups):
        if (table == g).any() or ambient_group == g:
            share = float((planes[g] != 0).any(axis=-1).mean())
            assert share > 0.05, (name, "plane", g, "non-zero share", share)
    for a in range(n_groups):
        for b in range(a + 1, n_groups):
            share = float((planes[a] != planes[b]).any(axis=-1).mean())
            assert share > 0.05, (name, "planes", a, b, "differing share", share)


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene dictionary, groups, ambient, noise or None, expected planes), computed once and
    read-only for every test."""
    make, groups, ambient, jitter = CASES[name]
    d = make()
    noise = noise_for(d, jitter)
    want = expected(d, groups, ambient, noise)
    table, n_groups, ambient_group = rtx.light_group_table(len(d["lights"]), groups, ambient)
    check_planes(name, table, n_groups, ambient_group, want)
    return d, groups, ambient, noise, want
