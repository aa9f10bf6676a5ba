"""Resolved buffers without a GPU: the C entry point's export and prototype, what
Scene.render_resolved refuses before any upload, the CLI's arguments and writers, and the
numpy resolve helper against a case worked by hand.

The module also holds the oracle of the resolved buffers, which tests/test_gpu_resolved.py
imports. Three steps: Scene.camera_rays gives every sample ray of the strip in fp32 (image row,
column, DOF origin, AA origin; replayed jitter applied), OracleScene.closest gives each ray's
first hit at each motion time, and `resolve` adds the samples' values in float32 in the
contract's order (DOF, AA, time; time fastest) -- a Python loop over the samples, vectorised
over the pixels -- and divides in float32. The albedo has a second oracle that does not pass
through camera_rays: OracleScene.render of the scene lit flat (`flat_lit`)."""
import copy
import os

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from rtx import main as cli
from oracle import oracle as O

f32 = np.float32

# ---------------------------------------------------------------- the oracle
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")


def resolve(hit, obj, depth, normal, albedo=None, matte=None):
    """The resolved buffers of P pixels from their S samples, sample-major: ``hit`` bool
    [S, ...], ``obj`` int [S, ...], ``depth`` float32 [S, ...], ``normal`` and ``albedo``
    float32 [S, ..., 3] (albedo may be None). ``matte``: object indices, or None. Every sum is
    float32 from +0 in sample order, a miss adds nothing, every quotient one float32 division;
    depth is +inf where no sample hits."""
    hit = np.asarray(hit, bool)
    S, shape = hit.shape[0], hit.shape[1:]
    nh = np.zeros(shape, np.int32)
    nm = np.zeros(shape, np.int32)
    dsum = np.zeros(shape, f32)
    nsum = np.zeros(shape + (3,), f32)
    asum = np.zeros(shape + (3,), f32)
    members = None if matte is None else np.unique(np.asarray(list(matte), np.int64))
    for s in range(S):
        h = hit[s]
        nh += h
        if members is not None:
            nm += h & np.isin(obj[s], members)
        dsum = np.where(h, dsum + np.asarray(depth[s], f32), dsum)
        nsum = np.where(h[..., None], nsum + np.asarray(normal[s], f32), nsum)
        if albedo is not None:
            asum = np.where(h[..., None], asum + np.asarray(albedo[s], f32), asum)
    ns = f32(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_depth = np.where(nh > 0, dsum / nh.astype(f32), f32(np.inf)).astype(f32)
    out = dict(alpha=nh.astype(f32) / ns, depth=mean_depth, normal=nsum / ns)
    if albedo is not None:
        out["albedo"] = asum / ns
    if members is not None:
        out["matte"] = nm.astype(f32) / ns
    assert all(v.dtype == f32 for v in out.values())
    return out


def sample_hits(d, sc, times, base=ASSETS, subimage=0, tasks=1):
    """The first hits of every sample of the strip, sample-major [S, H, W(, 3)]: a dict with
    hit, obj, mat, depth (float32) and normal. ``sc`` gives the rays (Scene.camera_rays: no
    jitter, or replayed jitter), ``times`` the motion times."""
    o, dr, group = sc.camera_rays(subimage, tasks)
    H, W = sc.vc.height, o.shape[0] // (sc.vc.height * group)
    osc = O.OracleScene(copy.deepcopy(d), base)
    per_time = [osc.closest(float(t), o, dr) for t in times]
    out = dict(hit=[], obj=[], mat=[], depth=[], normal=[])
    for g in range(group):
        for t, ob, _, m, nn, _ in per_time:
            pick = lambda a: a.reshape((H, W, group) + a.shape[1:])[:, :, g]  # noqa: E731
            out["hit"].append(pick(ob) >= 0)
            out["obj"].append(pick(ob))
            out["mat"].append(pick(m))
            out["depth"].append(pick(t.astype(f32)))
            out["normal"].append(pick(nn))
    return {k: np.stack(v) for k, v in out.items()}


def is_flat(d):
    """No hierarchy and no texture: a hit's albedo is its material's diffuse."""
    return not any(g["type"] == "node" or "texture" in g for g in d["objects"])


def expected(d, sc, times, base=ASSETS, subimage=0, tasks=1, matte=None):
    """(the resolved buffers' expected values in image layout, the samples). The albedo is
    there only for a flat scene, from the hit materials; `flat_lit` serves every scene."""
    s = sample_hits(d, sc, times, base, subimage, tasks)
    albedo = None
    if is_flat(d):
        diffuse = np.array([m.get("diffuse", [0, 0, 0]) for m in d["materials"]], np.float64).astype(f32)
        albedo = diffuse[np.maximum(s["mat"], 0)]
    return resolve(s["hit"], s["obj"], s["depth"], s["normal"], albedo, matte), s


def flat_lit(d, noise=None, subimage=0, tasks=1, base=ASSETS):
    """The albedo oracle: the scene lit flat (no lights, ambient 1, every material diffuse,
    diffuse <= 1) at the camera's full sampling, as float32 [H][W][3]. Each sample's colour is
    0 + 1 * diffuse, the clamp idle; the reference adds them in sample order and divides once."""
    d = copy.deepcopy(d)
    d["lights"] = []
    d["ambient"] = [1, 1, 1]
    for m in d["materials"]:
        m["type"] = "diffuse"
        assert all(0.0 <= float(x) <= 1.0 for x in m.get("diffuse", [0, 0, 0]))
    ref = O.OracleScene(d, base).render(subimage, tasks, noise=noise)
    return np.ascontiguousarray(np.swapaxes(ref, 0, 1)[::-1]).astype(f32)


def mixed_share(samples):
    """The share of the pixels whose samples do not all see the same object (-1: none)."""
    ob = samples["obj"]
    return float((ob != ob[0]).any(axis=0).mean())


def partial_share(a):
    """The share of the pixels with a value strictly between 0 and 1."""
    return float(((a > 0) & (a < 1)).mean())


# ---------------------------------------------------------------- tests
def test_entry_point_is_exported_and_the_abi_is_unchanged():
    lib = N.load()
    assert lib.rtx_abi_version() == 6 and N.ABI_VERSION == 6
    assert "rtx_render_resolved" in N.EXPORTS and hasattr(lib, "rtx_render_resolved")
    assert len(lib.rtx_render_resolved.argtypes) == 12
    assert lib.rtx_render_resolved.restype is N.C.c_int
    assert N.RTX_MATTE_MAX_OBJECTS == 256
    assert rtx.RESOLVED_NAMES == ("alpha", "matte", "depth", "normal", "albedo")
    assert "RESOLVED_NAMES" in rtx.__all__


def test_entry_point_checks_arguments_without_gpu():
    lib = N.load()
    assert lib.rtx_render_resolved(None, 0, 1, 0, None, None, None, None, None, None, 0, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_resolved: null scene" in lib.rtx_last_error()
    # (a null scene is refused whatever else is passed)
    ids = (N.C.c_int32 * 2)(0, 1)
    assert lib.rtx_render_resolved(None, -1, -1, -1, 16, 16, 16, 16, 16, ids, 2, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_resolved: null scene" in lib.rtx_last_error()


def test_render_resolved_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    n = len(sc.objects)
    assert 2 <= n < N.RTX_MATTE_MAX_OBJECTS
    for bad in (("object",), ("alpha", "position"), (), [], "coverage", ("alpha", "alpha")):
        with pytest.raises(ValueError):
            sc.render_resolved(bad)
    for kw in (dict(frame=1), dict(frame=-1), dict(windows=[0.0, 1.0], frame=2), dict(windows=[0.0, 1.0], frame=-1),
               dict(windows=[]), dict(windows=[[0.0, 1.0], [2.0]]), dict(row0=-1), dict(row0=4, nrows=3),
               dict(nrows=-1), dict(row0=7)):
        with pytest.raises(ValueError):
            sc.render_resolved(**kw)
    with pytest.raises(IndexError):  # (strip_columns, as render() raises it)
        sc.render_resolved(subimage=2, tasks=2)
    # "matte" needs its set: given, not empty, inside the scene's objects
    with pytest.raises(ValueError, match="matte"):
        sc.render_resolved(("alpha", "matte"))
    with pytest.raises(ValueError, match="matte"):
        sc.render_resolved(rtx.RESOLVED_NAMES)
    for bad in ([], (), [n], [-1], [0, n], [N.RTX_MATTE_MAX_OBJECTS], [0.5], [True], ["sphere"], [object()], 3, [None]):
        with pytest.raises(ValueError):
            sc.render_resolved(("matte",), matte=bad)
    # an object of another scene is not one of this scene's
    other = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    with pytest.raises(ValueError):
        sc.render_resolved(("matte",), matte=[other.objects[0]])
    # a good matte passes (objects by identity, indices, duplicates) and the call then fails on
    # its out tensor, still before any upload
    for good in ([0], [n - 1, 0, 0], [sc.objects[1]], [sc.objects[0], 1, np.int64(0)], (k for k in range(n))):
        with pytest.raises(ValueError, match="out"):
            sc.render_resolved(("alpha", "matte"), matte=good, out=dict(matte=torch.zeros((6, 8))))
    # a matte that is given is checked even when its buffer is not asked for
    with pytest.raises(ValueError):
        sc.render_resolved(("alpha",), matte=[n])
    bad_out = (
        dict(alpha=torch.zeros((6, 8), dtype=torch.float32)),                # not on the device
        dict(depth=torch.zeros((6, 8), dtype=torch.float64)),                # and not float32
        dict(normal=torch.zeros((6, 8), dtype=torch.float32)),               # and not [H, W, 3]
        dict(albedo=np.zeros((6, 8, 3), np.float32)),                        # not a tensor
        dict(position=torch.zeros((6, 8, 3), dtype=torch.float32)),          # an unknown name
        dict(matte=torch.zeros((6, 8), dtype=torch.float32)),                # not requested by default
    )
    for out in bad_out:
        with pytest.raises(ValueError):
            sc.render_resolved(out=out)
    assert sc._native is None  # nothing was uploaded


def test_matte_indices():
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(8, 6))
    idx = sc._matte_indices([sc.objects[2], 0, sc.objects[2]])
    assert idx.dtype == np.int32 and idx.flags.c_contiguous and list(idx) == [2, 0, 2]


def test_cli_resolved_arguments(capsys):
    a = cli.parse(["--infile", "s.json", "--resolved", "r.npz"])
    assert (a.resolved, a.resolved_names, a.matte_objects, a.rgba, a.outfile) == ("r.npz", None, None, None, "out.png")
    assert cli.resolved_names(a) == ("alpha", "depth", "normal", "albedo")
    a = cli.parse(["--infile", "s.json", "--resolved", "r.npz", "--matte-objects", "2", "0"])
    assert a.matte_objects == [2, 0] and cli.resolved_names(a) == ("alpha", "depth", "normal", "albedo", "matte")
    a = cli.parse(["--infile", "s.json", "--resolved", "r.npz", "--resolved-names", "matte", "alpha", "--matte-objects", "1"])
    assert cli.resolved_names(a) == ("matte", "alpha")
    a = cli.parse(["--infile", "s.json", "--resolved", "r.npz", "--aovs", "a.npz", "--occlusion", "o.npz", "--subimage", "1",
                   "--tasks", "2"])
    assert (a.resolved, a.aovs, a.occlusion, a.subimage, a.tasks) == ("r.npz", "a.npz", "o.npz", 1, 2)
    a = cli.parse(["--infile", "s.json", "--rgba", "c.png"])
    assert a.rgba == "c.png" and a.resolved is None
    a = cli.parse(["--infile", "s.json"])
    assert a.resolved is None and a.rgba is None and a.matte_objects is None   # the ordinary render is unchanged
    for bad, word in ((["--resolved", "r.npz", "--distributed"], "--distributed"),
                      (["--resolved", "r.npz", "--frames", "2"], "--frames"),
                      (["--resolved", "r.npz", "--panorama", "8", "4"], "--panorama"),
                      (["--rgba", "c.png", "--distributed"], "--distributed"),
                      (["--rgba", "c.png", "--frames", "2"], "--frames"),
                      (["--rgba", "c.png", "--panorama", "8", "4"], "--panorama"),
                      (["--rgba", "c.png", "--subimage", "0", "--tasks", "2"], "--subimage"),
                      (["--resolved", "r.npz", "--resolved-names", "alpha", "alpha"], "--resolved-names"),
                      (["--resolved", "r.npz", "--resolved-names", "position"], "--resolved-names"),
                      (["--resolved", "r.npz", "--resolved-names", "matte"], "--matte-objects"),
                      (["--resolved", "r.npz", "--resolved-names", "alpha", "--matte-objects", "0"], "--matte-objects"),
                      (["--resolved", "r.npz", "--matte-objects", "-1"], "--matte-objects"),
                      (["--resolved-names", "alpha"], "--resolved"),
                      (["--matte-objects", "0"], "--resolved")):
        with pytest.raises(SystemExit):
            cli.parse(["--infile", "s.json"] + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_writes_the_buffers(tmp_path, monkeypatch):
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(6, 4))
    seen = []

    def fake(buffers, matte=None, **kw):
        seen.append((tuple(buffers), matte, kw))
        return {n: torch.full((4, 6, 3) if n in ("normal", "albedo") else (4, 6), 0.25 * (k + 1), dtype=torch.float32)
                for k, n in enumerate(buffers)}
    monkeypatch.setattr(sc, "render_resolved", fake)
    path = str(tmp_path / "res")                                   # (the name is kept as given)
    args = cli.parse(["--infile", "s.json", "--resolved", path])
    assert cli.write_resolved(sc, args) == path
    with np.load(path) as z:
        assert sorted(z.files) == ["albedo", "alpha", "depth", "normal"]
        assert z["alpha"].dtype == np.float32 and z["alpha"].shape == (4, 6) and (z["alpha"] == 0.25).all()
        assert z["albedo"].shape == (4, 6, 3) and (z["albedo"] == 1.0).all()
    args = cli.parse(["--infile", "s.json", "--resolved", str(tmp_path / "r.npz"), "--subimage", "1", "--tasks", "3",
                      "--matte-objects", "2", "0"])
    cli.write_resolved(sc, args)
    with np.load(str(tmp_path / "r.npz")) as z:
        assert sorted(z.files) == ["albedo", "alpha", "depth", "matte", "normal"]
    args = cli.parse(["--infile", "s.json", "--resolved", str(tmp_path / "m.npz"), "--resolved-names", "matte",
                      "--matte-objects", "1"])
    cli.write_resolved(sc, args)
    with np.load(str(tmp_path / "m.npz")) as z:
        assert z.files == ["matte"]
    assert seen == [(("alpha", "depth", "normal", "albedo"), None, {}),
                    (("alpha", "depth", "normal", "albedo", "matte"), [2, 0], dict(subimage=1, tasks=3)),
                    (("matte",), [1], {})]


def test_rgba_image_keeps_the_rgb_bytes_and_adds_the_coverage(monkeypatch):
    """--rgba: RGB is --outfile's bytes untouched, A is the device conversion of alpha (here a
    host stand-in with rtx_fb_to_rgb8's rule, (v * 255.0) truncated)."""
    import rtx.scene
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(6, 4))
    alpha = torch.tensor(np.linspace(0.0, 1.0, 24, dtype=np.float32).reshape(4, 6))
    asked = []

    def fake(buffers, **kw):
        asked.append((tuple(buffers), kw))
        return dict(alpha=alpha)
    monkeypatch.setattr(sc, "render_resolved", fake)
    monkeypatch.setattr(rtx.scene, "fb_to_rgb8", lambda fb: (fb.double() * 255.0).to(torch.uint8))
    rgb = np.random.RandomState(3).randint(0, 256, (4, 6, 3)).astype(np.uint8)
    img = cli.rgba_image(rgb, sc)
    assert img.dtype == np.uint8 and img.shape == (4, 6, 4)
    assert np.array_equal(img[..., :3], rgb)
    assert np.array_equal(img[..., 3], (alpha.numpy().astype(np.float64) * 255.0).astype(np.uint8))
    assert img[0, 0, 3] == 0 and img[3, 5, 3] == 255
    assert asked == [(("alpha",), {})]


def test_resolve_by_hand():
    """Three samples of two pixels. Pixel 0 misses three times. Pixel 1: a hit on object 2
    (depth 1, normal (-0, 0.5, 1), albedo (0.25, 0.5, 1)), a miss, a hit on object 0 (depth 2,
    normal (-0, 0.25, 0), albedo (0.5, 0.5, 0))."""
    inf = np.inf
    hit = np.array([[False, True], [False, False], [False, True]])
    obj = np.array([[-1, 2], [-1, -1], [-1, 0]])
    depth = np.array([[inf, 1.0], [inf, inf], [inf, 2.0]], f32)
    normal = np.zeros((3, 2, 3), f32)
    normal[0, 1] = [-0.0, 0.5, 1.0]
    normal[2, 1] = [-0.0, 0.25, 0.0]
    albedo = np.zeros((3, 2, 3), f32)
    albedo[0, 1] = [0.25, 0.5, 1.0]
    albedo[2, 1] = [0.5, 0.5, 0.0]
    third, two_thirds = f32(1.0) / f32(3.0), f32(2.0) / f32(3.0)
    r = resolve(hit, obj, depth, normal, albedo, matte=[2, 2])
    assert all(v.dtype == np.float32 for v in r.values())
    assert np.array_equal(r["alpha"], np.array([0.0, two_thirds], f32))
    assert np.array_equal(r["matte"], np.array([0.0, third], f32))
    assert np.isposinf(r["depth"][0]) and r["depth"][1] == f32(1.5)          # a mean over the two hits
    assert np.array_equal(r["normal"], np.array([[0, 0, 0], [0.0, 0.25, third]], f32))  # means over all three
    assert np.array_equal(r["albedo"], np.array([[0, 0, 0], [0.25, third, third]], f32))
    assert not np.signbit(r["normal"]).any()                                  # +0 + -0 is +0
    # the matte of every object is the coverage; of an absent one, nothing
    assert np.array_equal(resolve(hit, obj, depth, normal, albedo, matte=[0, 1, 2])["matte"], r["alpha"])
    assert not resolve(hit, obj, depth, normal, albedo, matte=[1])["matte"].any()
    assert "matte" not in resolve(hit, obj, depth, normal, albedo) and "albedo" not in resolve(hit, obj, depth, normal)


def test_resolve_of_one_sample_is_the_sample():
    hit = np.array([[True, False, True]])
    obj = np.array([[4, -1, 0]])
    depth = np.array([[0.1, np.inf, 3.0]], f32)
    normal = np.array([[[-0.0, -1.0, 0.3], [0, 0, 0], [1.0, -0.0, 0.0]]], f32)
    r = resolve(hit, obj, depth, normal, normal, matte=[4])
    assert np.array_equal(r["alpha"], np.array([1, 0, 1], f32)) and np.array_equal(r["matte"], np.array([1, 0, 0], f32))
    assert np.array_equal(r["depth"], depth[0])
    assert np.array_equal(r["normal"], normal[0]) and np.array_equal(r["albedo"], normal[0])  # as values
    assert not np.signbit(r["normal"][normal[0] == 0]).any()                  # a -0 component is +0 after the sum


def test_sum_order_is_the_samples_order():
    """fp32 addition does not associate: 2^24 + 1 + 1 is 2^24 added in order, 2^24 + 2 otherwise."""
    big = f32(2.0 ** 24)
    depth = np.array([[big], [1.0], [1.0]], f32)
    hit = np.ones((3, 1), bool)
    zero = np.zeros((3, 1, 3), f32)
    r = resolve(hit, np.zeros((3, 1), int), depth, zero)
    assert r["depth"][0] == big / f32(3.0)
    r = resolve(hit, np.zeros((3, 1), int), depth[::-1], zero)
    assert r["depth"][0] == (big + f32(2.0)) / f32(3.0)
