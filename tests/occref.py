"""The occlusion pass (Scene.render_occlusion, rtx_render_occlusion) restated on the CPU: the
orthonormal frame of rtx.h in numpy fp32 (single IEEE operations, never fused, in the header's
order) and the two buffers from OracleScene.shadow for the hit points and normals the
first-hit pass stores."""
import copy

import numpy as np

from rtx import f32 as F

f32 = np.float32


def frame(n):
    """(T, U, n^) of normals [..., 3]: rtx.h's frame, operation for operation."""
    nh = F.normalize(np.asarray(n, f32))
    x, y, z = nh[..., 0], nh[..., 1], nh[..., 2]
    s = np.copysign(f32(1.0), z)
    a = f32(-1.0) / (s + z)
    b = (x * y) * a
    T = np.stack([f32(1.0) + ((s * x) * x) * a, s * b, -(s * x)], axis=-1)
    U = np.stack([b, s + ((y * y) * a), -y], axis=-1)
    assert T.dtype == f32 and U.dtype == f32 and nh.dtype == f32
    return T, U, nh


def ao_rays(n, dirs):
    """d_k = ((x_k * T) + (y_k * U)) + (z_k * n^) for normals [m, 3] and local directions
    [K, 3]: float32 [m, K, 3]."""
    T, U, nh = frame(n)
    dirs = np.asarray(dirs, f32)
    x, y, z = (dirs[None, :, c, None] for c in range(3))
    d = ((x * T[:, None, :]) + (y * U[:, None, :])) + (z * nh[:, None, :])
    assert d.dtype == f32
    return d


def light_rays(lights, p):
    """Per light of the scene (rtx.helperclasses.Light): (directions [m, 3] fp32, t_max) of its
    shadow rays from the points p (scene.py:150-158)."""
    p = np.asarray(p, f32)
    out = []
    for L in lights:
        v = np.asarray(L.vector, f32)
        if L.type == "point":
            out.append((v - p, 1.0))
        else:
            out.append((np.broadcast_to(-v, p.shape).copy(), np.inf))
    return out


def expected(oracle, lights, aov, time, dirs=None, radius=np.inf):
    """The buffers' expected values from first-hit buffers `aov` (host arrays "depth",
    "position", "normal" of one camera state): (lights uint32 [H, W], ao float32 [H, W] or None,
    hit mask)."""
    hit = np.isfinite(aov["depth"])
    p = np.ascontiguousarray(aov["position"][hit])
    n = np.ascontiguousarray(aov["normal"][hit])
    mask = np.zeros(len(p), np.uint32)
    for i, (d, tm) in enumerate(light_rays(lights, p)[:32]):  # (the mask holds 32 lights)
        free = oracle.shadow(time, p, d, tm) == 0
        mask |= np.where(free, np.uint32(1 << i), np.uint32(0)).astype(np.uint32)
    want_l = np.zeros(hit.shape, np.uint32)
    want_l[hit] = mask
    want_a = None
    if dirs is not None:
        K = len(dirs)
        d = ao_rays(n, dirs)
        free = oracle.shadow(time, np.repeat(p, K, axis=0), d.reshape(-1, 3), radius) == 0
        u = free.reshape(len(p), K).sum(axis=1)
        want_a = np.ones(hit.shape, f32)
        want_a[hit] = u.astype(f32) / f32(K)
    return want_l, want_a, hit


def oracle_scene(d, base):
    from oracle import oracle as O
    return O.OracleScene(copy.deepcopy(d), base)
