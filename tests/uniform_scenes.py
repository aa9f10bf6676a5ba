"""Scenes for the wave-uniform hit tests (tests/test_unlit_uniform.py, tests/test_gpu_unlit_uniform.py):
TwoSpheresPlane with a camera whose tiny frames hold every class of 8x8 tile, variations of its
materials and lights that make a wrong word of a literal material record visible (both checker
materials black, -0.0, specular only, negative light colours, a light on the plane), boxes,
one object more than the per-object shading copies (rtx_trace.h kUniformHitMax), a moving sphere."""
import copy

import numpy as np

from rtx.io import bundled_scene_dict

ONE = {"jitter": False, "samples": 1}
RES = [(64, 48), (70, 45)]  # whole tiles; edge tiles in both directions
CAP = 4  # rtx_trace.h kUniformHitMax
BLACK, WHITE = 2, 3  # TwoSpheresPlane's checker materials


def tsp(res=(64, 48)):
    d = bundled_scene_dict("TwoSpheresPlane", resolution=list(res))
    d.pop("__base_dir__", None)
    d["AA"] = dict(ONE)
    # close and wide: sky above the horizon, checker squares larger than a tile in front
    d["camera"] = {"fov": 60.0, "lookAt": [0.0, 1.0, -0.5], "position": [0.3, 2.0, 2.5], "up": [0.0, 1.0, 0.0]}
    return d


def _mat(d, i, **kw):
    d["materials"][i] = dict(d["materials"][i], **kw)


def scenes(res=(64, 48)):
    """name -> scene dict."""
    out = {"tsp": tsp(res)}
    d = tsp(res)
    _mat(d, WHITE, diffuse=[0.0, 0.0, 0.0])
    out["both_unlit"] = d
    d = tsp(res)
    d["objects"][0]["materials"] = [BLACK]
    out["one_material"] = d
    d = tsp(res)
    _mat(d, BLACK, specular=[0.3, 0.2, 0.1], hardness=8)
    out["zero_diffuse_specular"] = d
    d = tsp(res)
    _mat(d, BLACK, diffuse=[-0.0, 0.0, -0.0])
    out["negative_zero_diffuse"] = d
    d = tsp(res)
    d["lights"][0]["colour"] = [-0.8, 0.2, -0.2]
    out["negative_light"] = d
    d = tsp(res)
    d["lights"][1]["position"] = light_on_plane(res)
    out["light_on_plane"] = d
    d = tsp(res)
    d["lights"][1] = {"name": "sun", "type": "directional", "direction": [0.4, -1.0, -0.3], "colour": [0.8, 0.8, 0.8],
                      "power": 0.7}
    out["directional"] = d
    d = tsp(res)
    d["objects"][2] = {"name": "box0", "type": "box", "position": [1.2, 0.5, 0.3], "size": [1.0, 1.0, 1.2], "materials": [0]}
    out["box"] = d
    d = tsp(res)
    d["objects"] += [{"name": "s2", "type": "sphere", "position": [1.8, 0.4, 0.8], "radius": 0.4, "materials": [3]},
                     {"name": "s3", "type": "sphere", "position": [-2.2, 0.3, 1.2], "radius": 0.3, "materials": [0]}]
    assert len(d["objects"]) == CAP + 1
    out["over_cap"] = d
    d = tsp(res)
    d["objects"][2]["speed"] = [0.4, 0.1, -0.3]
    d["motion"] = {"time": 0.75, "samples": 1, "final": 1}  # one motion time, not 0
    out["moving"] = d
    return out


def light_on_plane(res):
    """The fp32 hit point of one black checker pixel of tsp(res): a point light exactly there has
    a zero shadow direction at that pixel."""
    import hostemu
    from common import product_scene_dict
    sc = product_scene_dict(tsp(res))
    o, dr, _ = primary_rays(sc)
    hit = hostemu.intersect(sc, o, dr)
    k = np.flatnonzero((hit["obj"] == 0) & (hit["mat"] == BLACK))
    k = k[len(k) // 2]
    return [float(x) for x in hit["position"][k]]


def bundled(name, res):
    d = bundled_scene_dict(name, resolution=list(res))
    d.pop("__base_dir__", None)
    d["AA"] = dict(ONE)
    return d


def primary_rays(sc):
    """The pinhole primary rays of a product scene as the device builds them (fp32), one per
    pixel, and each pixel's (tile row, tile column) in the output block."""
    cd, t = sc.camera_desc()
    W, H = cd.ncols, cd.height
    f32 = np.float32
    u, v, w = (np.asarray(x, f32) for x in (sc.vc.u, sc.vc.v, sc.vc.w))
    xs, ys = np.asarray(t["xs"], f32), np.asarray(t["ys"], f32)
    cc, jj = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    base = xs[cc][..., None] * u + ys[jj][..., None] * v - w * f32(sc.vc.d)
    dr = (base / np.linalg.norm(base, axis=-1, keepdims=True).astype(f32)).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(sc.vc.position, f32), dr.shape)
    tiles = np.stack([((H - 1 - jj) >> 3).ravel(), (cc >> 3).ravel()], axis=1)
    return np.ascontiguousarray(o), np.ascontiguousarray(dr), tiles


def tile_classes(d):
    """Counts of the 8x8 tiles of scene d's frame by what their primary rays hit (host
    emulation of closest_hit): all-miss, hit + miss, one object, two objects, all-unlit (every
    hit the black material), lit/unlit mixed."""
    import hostemu
    from common import product_scene_dict
    sc = product_scene_dict(copy.deepcopy(d))
    o, dr, tiles = primary_rays(sc)
    hit = hostemu.intersect(sc, o, dr)
    unlit = {i for i, m in enumerate(d["materials"])
             if all(x == 0 and not np.signbit(x) for x in list(m["diffuse"]) + list(m["specular"]))}
    cls = dict(all_miss=0, hit_miss=0, one_object=0, two_objects=0, all_unlit=0, mixed_lit=0)
    key = tiles[:, 0] * 4096 + tiles[:, 1]
    for k in np.unique(key):
        sel = key == k
        ob, mt = hit["obj"][sel], hit["mat"][sel]
        objs = set(ob[ob >= 0].tolist())
        dark = np.array([m in unlit for m in mt[ob >= 0]], bool)
        cls["all_miss"] += not objs
        cls["hit_miss"] += bool(objs) and bool((ob < 0).any())
        cls["one_object"] += len(objs) == 1
        cls["two_objects"] += len(objs) == 2
        cls["all_unlit"] += bool(objs) and bool(dark.all())
        cls["mixed_lit"] += bool(dark.any()) and not dark.all()
    return cls
