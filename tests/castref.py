"""Tests-only: probe rays for Scene.cast_rays and their colours by the reference's own function,
oracle/pyloop.py's PyLoopScene.cast_ray (scene.py:81-116), one ray and motion time at a time."""
import copy
import os

import numpy as np

from oracle import oracle as O
from oracle import pyloop as P
from rtx import f32 as F

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")
f32 = np.float32


def bundle(name, res=(16, 12), **edits):
    """The bundled scene's description at a small resolution (cast_rays reads no camera)."""
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


def probe_rays(d, n, seed=7):
    """n rays [n, 3] fp32 for the scene description d, in thirds: from the camera position
    toward lookAt + U(-3, 3)^3; from lookAt + U(-4, 4)^3 along normal-distributed directions;
    from within 0.2 of the position of every top-level sphere, box, node and mesh in turn
    (inside the shapes) along normal-distributed directions. 75 % of the directions are
    normalised in fp32, the others keep their length."""
    rs = np.random.RandomState(seed)
    pos = np.asarray(d["camera"]["position"], np.float64)
    look = np.asarray(d["camera"]["lookAt"], np.float64)
    k = n // 3
    m = n - 2 * k
    o1 = np.broadcast_to(pos, (k, 3))
    d1 = look + rs.uniform(-3, 3, (k, 3)) - pos
    o2 = look + rs.uniform(-4, 4, (k, 3))
    d2 = rs.normal(size=(k, 3))
    centres = np.asarray([g["position"] for g in d["objects"]
                          if g["type"] in ("sphere", "box", "node", "mesh") and "position" in g], np.float64)
    assert len(centres) > 0
    o3 = centres[np.arange(m) % len(centres)] + rs.uniform(-0.2, 0.2, (m, 3))
    d3 = rs.normal(size=(m, 3))
    o = np.concatenate([o1, o2, o3]).astype(f32)
    dd = np.concatenate([d1, d2, d3]).astype(f32)
    unit = rs.rand(n) < 0.75
    dd[unit] = F.normalize(dd[unit])
    assert 0.6 < unit.mean() < 0.9
    return np.ascontiguousarray(o), np.ascontiguousarray(dd)


class Reference:
    """PyLoopScene.cast_ray over rays and times: colours [n][T][3] fp32, and per cast the
    number of levels it took (the depth of the recursion: 1 = no secondary ray)."""

    def __init__(self, d, base=ASSETS):
        self.ps = P.PyLoopScene(O.OracleScene(copy.deepcopy(d), base))
        inner = self.ps.cast_ray
        self._deepest = 0

        def counted(o, dd, max_recursion=10, in_shape=False):
            if max_recursion > 0:  # (cast_ray(max_recursion=0) returns black without a cast)
                self._deepest = max(self._deepest, 11 - max_recursion)
            return inner(o, dd, max_recursion, in_shape)

        self.ps.cast_ray = counted  # the recursion goes through self.cast_ray: every level is seen

    def cast(self, o, dd, times):
        n, T = len(o), len(times)
        rgb = np.zeros((n, T, 3), f32)
        levels = np.zeros((n, T), np.int32)
        for i in range(n):
            for k, t in enumerate(times):
                self.ps.current_time = float(t)  # a Python float, as render()'s loop sets it
                self._deepest = 0
                rgb[i, k] = self.ps.cast_ray(P.V(*o[i]), P.V(*dd[i]))
                levels[i, k] = self._deepest
        return rgb, levels


def ordered_mean(c, group):
    """c [n][T][3] fp32 -> [n / group][3]: the samples of each output added in order (ray,
    then time) in fp32 from +0, then one fp32 division by fl32(S)."""
    n, T = c.shape[:2]
    S = group * T
    c = c.reshape(n // group, S, 3)
    acc = np.zeros((n // group, 3), f32)
    for s in range(S):
        acc = acc + c[:, s]
    return acc / f32(S)
