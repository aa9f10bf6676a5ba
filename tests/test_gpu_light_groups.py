"""Light groups (Scene.render_light_groups, rtx_render_light_groups) on the GPU, bit for bit
against the oracle: plane g is OracleScene's render of the scene description edited to hold only
group g's lights and, unless g is the ambient's group, a zero ambient (tests/lightgroups.py).
Every comparison is np.array_equal on float32; an expectation is computed once per case."""
import copy

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from common import OPTS, product_scene_dict
import castref
import lightgroups as LG
from test_gpu_aov import bundle

pytestmark = pytest.mark.gpu

RES = LG.RES


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def scene(name):
    """The product's scene of a case: it draws Philox jitter itself and replays a seeded stream."""
    d, groups, ambient, noise, want = LG.case(name)
    sc = product_scene_dict(d)
    if LG.CASES[name][3] not in (None, "philox"):
        sc.jitter_noise = noise
    return sc, groups, ambient, want


def same(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    for g in range(len(want)):
        assert np.array_equal(got[g], want[g]), (what, "plane", g, float((got[g] != want[g]).any(axis=-1).mean()))


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(LG.CASES))
def test_planes_match_the_oracle(name):
    sc, groups, ambient, want = scene(name)
    got = host(sc.render_light_groups(groups, ambient))
    H, W = sc.vc.height, sc.vc.width
    assert got.shape == (len(want), H, W, 3)
    same(got, want, name)
    # what keeps the case from being vacuous, on the oracle's values and the scene's own
    if name == "tsp":
        assert sc.samples == 3 and len(sc.lights) == 2 and len(want) == 3
    if name == "mirror2":
        assert (want == 1.0).any(axis=(1, 2, 3)).any(), "no clamp engaged"
        o, dd, group = sc.camera_rays()
        assert group == 1
        pick = np.arange(0, len(o), 7)  # every seventh pixel: the reference's cast_ray is a Python loop
        _, levels = castref.Reference(LG.case(name)[0]).cast(o[pick], dd[pick], [0.0])
        assert levels.max() >= 3, levels.max()
    if name == "torus":
        assert len(sc.lights) == 3 and any(ob.__class__.__name__ == "Mesh" for ob in sc.objects)
    if name == "motionblur2":
        assert len(sc.vc.motion_times) == 17 and len(want) == 2
    if name.startswith("dof"):
        assert (sc.vc.dof_samples, sc.samples) == (3, 2) and sc.jitter
        assert (sc.jitter_noise is None) == (name == "dof_philox")
    if name == "excluded":
        assert len(want) == 1 and len(sc.lights) == 2
        # the plane is not the beauty image: light 1 is missing from it
        assert not np.array_equal(want[0], LG.expected(LG.case(name)[0], [[0, 1]], 0)[0])
    if name == "nolights":
        assert len(sc.lights) == 0 and len(want) == 1


@pytest.mark.parametrize("name", ["tsp", "mirror2", "torus", "dof_philox"])
def test_one_group_of_everything_is_the_render(name, monkeypatch):
    """No oracle: one group with every light and the ambient is render_device's framebuffer
    (through the generic render kernel: no compile of a specialized one)."""
    monkeypatch.setattr(OPTS, "jit", "0")
    sc, _, _, _ = scene(name)
    img = sc.render_device().clone()
    got = sc.render_light_groups([list(range(len(sc.lights)))], 0)
    assert got.shape == (1,) + tuple(img.shape)
    assert torch.equal(got[0], img)
    assert float(img.max()) > 0.0


# ---------------------------------------------------------------- rows, strips, sequences, out
def test_row_blocks_and_strips():
    sc, groups, ambient, want = scene("dof_philox")
    W = sc.vc.width
    full = host(sc.render_light_groups(groups, ambient))
    same(full, want, "full")
    rows = host(sc.render_light_groups(groups, ambient, row0=5, nrows=19))  # off the 8-row grid
    same(rows, want[:, 5:24], "rows")
    col0, ncols = rtx.strip_columns(W, 1, 3)
    part = host(sc.render_light_groups(groups, ambient, subimage=1, tasks=3))
    same(part, want[:, :, col0:col0 + ncols], "strip")
    assert sc.render_light_groups(groups, ambient, row0=5, nrows=0).shape == (3, 0, W, 3)


def test_sequence_frame():
    """frame=1 of a two-window sequence: the second window holds the case's own motion times, so
    the oracle's render of the case is the oracle at that window's times."""
    sc, groups, ambient, want = scene("motionblur2")
    own = [float(t) for t in sc.vc.motion_times]
    windows = [[t + 0.3 for t in own], own]
    got = host(sc.render_light_groups(groups, ambient, windows=windows, frame=1))
    same(got, want, "frame 1")
    other = host(sc.render_light_groups(groups, ambient, windows=windows, frame=0))
    assert not np.array_equal(other, got)  # the scene moves
    with pytest.raises(ValueError):
        sc.render_light_groups(groups, ambient, windows=windows, frame=2)


def test_out_tensor_and_empty_groups():
    sc, groups, ambient, want = scene("tsp")
    H, W = sc.vc.height, sc.vc.width
    out = torch.full((3, H, W, 3), float("nan"), device="cuda")
    got = sc.render_light_groups(groups, ambient, out=out)
    assert got is out
    same(host(out), want, "out")
    with pytest.raises(ValueError, match="out"):
        sc.render_light_groups(groups, ambient, out=torch.empty((3, H, 3, W), device="cuda").transpose(2, 3))
    # G = 8: group 3 holds everything, the seven others are empty and stay black
    eight = [[], [], [], [0, 1], [], [], [], []]
    out8 = torch.full((8, H, W, 3), float("nan"), device="cuda")
    g8 = host(sc.render_light_groups(eight, 3, out=out8))
    beauty = LG.expected(LG.case("tsp")[0], [[0, 1]], 0)[0]
    assert np.array_equal(g8[3], beauty)
    for g in (0, 1, 2, 4, 5, 6, 7):
        assert not g8[g].any() and not np.signbit(g8[g]).any(), g
    # five groups take the eight-plane kernel too: the lights apart, the ambient in group 4
    five = host(sc.render_light_groups([[1], [], [0], []], "own"))
    assert np.array_equal(five[0], want[1]) and np.array_equal(five[2], want[0]) and np.array_equal(five[4], want[2])
    assert not five[1].any() and not five[3].any()


def test_graph_replay():
    """A call captured after one eager call replays to the same bytes (a sequential capture)."""
    sc, groups, ambient, want = scene("mirror2")
    out = torch.empty((2, sc.vc.height, sc.vc.width, 3), device="cuda")
    sc.render_light_groups(groups, ambient, out=out)
    same(host(out), want, "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        sc.render_light_groups(groups, ambient, out=out)
    for _ in range(2):
        out.zero_()
        g.replay()
        same(host(out), want, "replay")


def test_uniform_hit_does_not_matter(monkeypatch):
    _, groups, ambient, want = scene("tsp")
    for v in ("0", "1"):
        monkeypatch.setattr(OPTS, "uniform_hit", v)
        same(host(product_scene_dict(LG.case("tsp")[0]).render_light_groups(groups, ambient)), want, "uniform_hit " + v)


# ---------------------------------------------------------------- the entry point's errors
def test_entry_point_argument_errors():
    lib = N.load()
    sc = product_scene_dict(bundle("TwoSpheresPlane", (16, 8)))
    h = sc.native().h
    buf = torch.full((3 * 16 * 8 * 3,), float("nan"), device="cuda")
    p = buf.data_ptr()
    ints = lambda *v: (N.C.c_int32 * len(v))(*v)  # noqa: E731
    t01 = ints(0, 1)

    def call(row0, nrows, frame, table, n_groups, ambient_group, out, scene=h):
        return lib.rtx_render_light_groups(scene, row0, nrows, frame, table, n_groups, ambient_group, out, None)

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(buf).all())
    assert call(0, 8, 0, t01, 2, -1, p) == N.RTX_ERR_STATE
    assert b"rtx_render_light_groups: rtx_camera_set" in lib.rtx_last_error() and untouched()
    sc._set_camera(0, 1)
    bad = [(0, 9, 0, t01, 2, -1, p), (-1, 2, 0, t01, 2, -1, p), (4, -1, 0, t01, 2, -1, p), (7, 2, 0, t01, 2, -1, p),
           (0, 8, 0, t01, 2, -1, None), (0, 8, 0, None, 2, -1, p), (0, 8, 1, t01, 2, -1, p), (0, 8, -1, t01, 2, -1, p),
           (0, 8, 0, t01, 0, -1, p), (0, 8, 0, t01, -1, -1, p), (0, 8, 0, ints(0, 0), 9, -1, p),
           (0, 8, 0, ints(0, 2), 2, -1, p), (0, 8, 0, ints(-2, 1), 2, -1, p), (0, 8, 0, t01, 2, 2, p),
           (0, 8, 0, t01, 2, -2, p), (3, 0, 0, t01, 2, 5, p)]
    for args in bad:
        assert call(*args) == N.RTX_ERR_INVALID, args[:3] + args[4:6]
        assert lib.rtx_last_error().startswith(b"rtx_render_light_groups: "), args[:3]
    assert call(0, 8, 0, t01, 2, -1, p, scene=None) == N.RTX_ERR_INVALID
    assert b"rtx_render_light_groups: null scene" in lib.rtx_last_error()
    assert untouched()  # no refused call wrote anything
    assert call(8, 0, 0, t01, 2, -1, p) == N.RTX_OK and untouched()  # no rows: nothing to do
    assert sc.last_kernel == ""  # rtx_last_kernel is left as it is
    # more lights than the word of free lights holds
    d = bundle("TwoSpheresPlane", (16, 8))
    d["lights"] = [copy.deepcopy(d["lights"][k % 2]) for k in range(33)]
    many = product_scene_dict(d)
    many._set_camera(0, 1)
    assert call(0, 8, 0, ints(*([0] * 33)), 1, 0, p, scene=many.native().h) == N.RTX_ERR_INVALID
    assert b"32 lights" in lib.rtx_last_error() and untouched()
    # a hierarchy / texture scene
    ns2 = product_scene_dict(bundle("NovelScene2", (16, 8)))
    ns2._set_camera(0, 1)
    table = ints(*([0] * max(1, len(ns2.lights))))
    assert call(0, 8, 0, table, 1, 0, p, scene=ns2.native().h) == N.RTX_ERR_UNSUPPORTED
    assert b"hierarchies or textures" in lib.rtx_last_error() and untouched()
    with pytest.raises(N.RtxError, match="hierarchies or textures"):
        ns2.render_light_groups([list(range(len(ns2.lights)))], 0)
    # and a good call fills exactly its planes
    assert call(0, 8, 0, t01, 2, -1, p) == N.RTX_OK
    torch.cuda.synchronize()
    filled = torch.isnan(buf).view(3, -1)
    assert not bool(filled[:2].any()) and bool(filled[2].all())
