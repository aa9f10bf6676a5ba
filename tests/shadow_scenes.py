"""Random flat scenes (reference JSON schema) for the shadow-bin tests: planes, spheres and
boxes of diffuse materials under one to eight lights, one sample per pixel (the cameras that
get shadow bins)."""
import numpy as np


def flat_scene(seed, res=(96, 72), points_only=False):
    """kind by seed % 4 -- 0: plain; 1: the camera inside a large sphere; 2: one moving sphere
    (two motion times); 3: a narrow or a very wide field of view. Lights: point and (unless
    points_only, which also leaves the boxes out: the scenes of the all-lights-at-once shadow
    test) directional; below the ground, inside a sphere, between the camera and the objects.
    Spheres rest on the ground (touching it) or float; boxes stand on it or float."""
    rng = np.random.RandomState(31000 + seed)
    r = lambda lo, hi, n=None: np.round(rng.uniform(lo, hi, n), 3).tolist()  # noqa: E731
    kind = seed % 4
    mats = [{"name": "m%d" % i, "ID": i, "type": "diffuse", "diffuse": r(0.1, 1, 3), "specular": r(0, 1, 3),
             "hardness": int(rng.choice([0, 16, 50]))} for i in range(4)]
    objs = [{"name": "ground", "type": "plane", "normal": [0.0, 1.0, 0.0], "position": [0.0, -1.0, 0.0],
             "materials": [0, 1]}]
    if rng.rand() < 0.4:  # a wall behind the objects, facing the camera
        objs.append({"name": "wall", "type": "plane", "normal": [float(r(-0.3, 0.3)), 0.0, 1.0],
                     "position": [0.0, 0.0, float(r(-9, -6))], "materials": [int(rng.randint(4))]})
    spheres = []
    for k in range(rng.randint(2, 6)):
        rad = float(r(0.2, 1.0))
        pos = r(-3, 3, 3)
        if rng.rand() < 0.5:
            pos[1] = round(-1.0 + rad, 3)  # touching the ground
        o = {"name": "s%d" % k, "type": "sphere", "radius": rad, "position": pos, "materials": [int(rng.randint(4))]}
        spheres.append(o)
        objs.append(o)
    if kind == 2:
        spheres[0]["speed"] = r(-0.6, 0.6, 3)
    if kind == 1:
        objs.append({"name": "dome", "type": "sphere", "radius": 40.0, "position": [0.0, 0.0, 0.0],
                     "materials": [int(rng.randint(4))]})
    if not points_only:
        for k in range(rng.randint(0, 4)):
            sz = r(0.3, 1.5, 3)
            pos = r(-3, 3, 3)
            if rng.rand() < 0.5:
                pos[1] = round(-1.0 + sz[1] / 2, 3)
            objs.append({"name": "b%d" % k, "type": "box", "position": pos, "size": sz, "materials": [int(rng.randint(4))]})
    cam = [float(r(-2, 2)), float(r(0.5, 4)), float(r(6, 9))]
    lights = []
    for i in range(rng.randint(1, 9)):
        u = rng.rand()
        if not points_only and u < 0.3:
            lights.append({"name": "d%d" % i, "type": "directional",
                           "direction": [float(r(-1, 1)), float(r(-1, 0.2)), float(r(-1, 1))], "colour": r(0.2, 1, 3),
                           "power": float(r(0.2, 0.8))})
            continue
        if u < 0.4:  # inside a sphere
            pos = list(spheres[int(rng.randint(len(spheres)))]["position"])
        elif u < 0.5:  # under the ground
            pos = [float(r(-3, 3)), float(r(-4, -1.5)), float(r(-3, 3))]
        elif u < 0.65:  # between the camera and the objects
            pos = [round(0.5 * c, 3) for c in cam]
        else:
            pos = r(-8, 8, 3)
            pos[1] = abs(pos[1]) + 1.0
        lights.append({"name": "p%d" % i, "type": "point", "position": pos, "colour": r(0.2, 1, 3), "power": float(r(0.2, 1.0))})
    fov = float(rng.choice([15.0, 120.0])) if kind == 3 else float(r(35, 75))
    sc = {"resolution": list(res), "AA": {"jitter": False, "samples": 1}, "ambient": [0.1, 0.1, 0.1],
          "camera": {"position": cam, "lookAt": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "fov": fov},
          "materials": mats, "objects": objs, "lights": lights}
    if kind == 2:
        sc["motion"] = {"time": 1.0, "samples": 1, "final": 1}
    return sc


# (camera, point light, sphere centre, radius): a sphere beside the edge of a tile's hull from
# its bottom-left ground hit to the light, with a radius inside the ~2e-6 wide window between
# the fp64 distance of its centre to that edge and the radius from which the device's fp32
# shadow ray of that pixel meets it (found by bisection on the CPU, then centred in the window).
TANGENT_CASES = [
    ([1.0, 3.0, 7.0], [5.0, 6.0, 2.0], [1.977, 3.229, 2.824], 0.5001149408),
    ([1.0, 3.0, 7.0], [-4.0, 5.0, 3.0], [-2.032, 2.283, 3.237], 0.5001906982),
    ([1.0, 3.0, 7.0], [2.0, 7.0, -3.0], [1.031, 4.774, -1.632], 0.5002074812),
]


def tangent_scene(case, res=(32, 32)):
    cam, light, centre, radius = TANGENT_CASES[case]
    return {"resolution": list(res), "AA": {"jitter": False, "samples": 1}, "ambient": [0.1, 0.1, 0.1],
            "camera": {"position": cam, "lookAt": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "fov": 45.0},
            "materials": [{"name": "m", "ID": 0, "type": "diffuse", "diffuse": [0.8, 0.8, 0.8], "specular": [0, 0, 0],
                           "hardness": 0}],
            "objects": [{"name": "ground", "type": "plane", "normal": [0.0, 1.0, 0.0], "position": [0.0, 0.0, 0.0],
                         "materials": [0]},
                        {"name": "s", "type": "sphere", "radius": radius, "position": list(centre), "materials": [0]}],
            "lights": [{"name": "p", "type": "point", "position": light, "colour": [1, 1, 1], "power": 1.0}]}
