"""Light groups (Scene.render_light_groups, rtx_render_light_groups) without a GPU: the table that
turns the Python arguments into the entry point's arrays, the export and its binding, and
the tests' own expectation (tests/lightgroups.py) against the oracle."""
import copy

import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from oracle import oracle as O
import lightgroups as LG
from test_gpu_aov import bundle


# ---------------------------------------------------------------- light_group_table
def test_table_defaults_and_ambient():
    t, g, a = rtx.light_group_table(3)
    assert t.dtype == np.int32 and t.flags.c_contiguous and list(t) == [0, 1, 2] and (g, a) == (4, 3)  # "own": last
    t, g, a = rtx.light_group_table(3, ambient=None)
    assert list(t) == [0, 1, 2] and (g, a) == (3, -1)
    t, g, a = rtx.light_group_table(3, [[2], [0]], ambient=1)
    assert list(t) == [1, -1, 0] and (g, a) == (2, 1)  # light 1 is in no group
    t, g, a = rtx.light_group_table(3, [[0, 1, 2]], ambient=0)
    assert list(t) == [0, 0, 0] and (g, a) == (1, 0)
    t, g, a = rtx.light_group_table(2, ([], (1,), []), "own")
    assert list(t) == [-1, 1] and (g, a) == (4, 3)  # empty groups keep their planes
    t, g, a = rtx.light_group_table(0, [[]], 0)
    assert t.shape == (0,) and (g, a) == (1, 0)  # a scene without lights
    t, g, a = rtx.light_group_table(0)
    assert t.shape == (0,) and (g, a) == (1, 0)  # its only plane is the ambient's own
    t, g, a = rtx.light_group_table(8, [[k] for k in range(7)] + [[]], np.int64(7))
    assert (g, a) == (8, 7) and list(t) == [0, 1, 2, 3, 4, 5, 6, -1]
    assert "light_group_table" in rtx.__all__ and N.RTX_LIGHT_GROUPS_MAX == 8


@pytest.mark.parametrize("n,groups,ambient", [
    (2, [[0], [0]], None),              # a light in two groups
    (2, [[0, 0]], None),                # ... or twice in one
    (2, [[2]], None),                   # a light index out of range
    (2, [[-1]], None),
    (2, [[0.0]], None),
    (2, [[True]], None),
    (2, 3, None),                       # not a sequence of sequences
    (2, [0, 1], None),
    (8, None, "own"),                   # nine groups with the ambient's own
    (9, None, None),                    # nine groups
    (2, [], None),                      # no group at all
    (0, None, None),
    (2, [[0], [1]], 2),                 # the ambient's group out of range
    (2, [[0], [1]], -1),
    (2, [[0], [1]], "group0"),
    (2, [[0], [1]], 0.0),
    (2, [[0], [1]], True),
])
def test_table_refuses(n, groups, ambient):
    with pytest.raises(ValueError):
        rtx.light_group_table(n, groups, ambient)


# ---------------------------------------------------------------- the entry point and the method
def test_entry_point_is_exported_and_the_abi_is_unchanged():
    lib = N.load()
    assert lib.rtx_abi_version() == 6 and N.ABI_VERSION == 6
    assert "rtx_render_light_groups" in N.EXPORTS and hasattr(lib, "rtx_render_light_groups")
    assert len(lib.rtx_render_light_groups.argtypes) == 9
    assert lib.rtx_render_light_groups.restype is N.C.c_int
    # a null scene is refused whatever else is passed, before any HIP call
    table = (N.C.c_int32 * 2)(0, 1)
    assert lib.rtx_render_light_groups(None, 0, 1, 0, table, 2, -1, 16, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_light_groups: null scene" in lib.rtx_last_error()
    assert lib.rtx_render_light_groups(None, -1, -1, -1, None, 0, 9, None, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_light_groups: null scene" in lib.rtx_last_error()


def test_render_light_groups_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("TwoSpheresPlane", resolution=(8, 6))
    assert len(sc.lights) == 2
    for kw in (dict(groups=[[0], [0]]), dict(groups=[[2]]), dict(groups=[], ambient=None), dict(groups=[[]] * 8),
               dict(groups=[[]] * 9, ambient=None), dict(ambient=3), dict(ambient="none"),
               dict(frame=1), dict(windows=[0.0, 1.0], frame=2), dict(row0=-1), dict(row0=4, nrows=3), dict(nrows=-1)):
        with pytest.raises(ValueError):
            sc.render_light_groups(**kw)
    with pytest.raises(IndexError):  # (strip_columns, as render() raises it)
        sc.render_light_groups(subimage=2, tasks=2)
    for out in (torch.zeros((3, 6, 8, 3)),                                # not on the device
                torch.zeros((2, 6, 8, 3)),                                # and not G planes
                torch.zeros((3, 6, 8, 3), dtype=torch.float64),           # and not float32
                np.zeros((3, 6, 8, 3), np.float32)):                      # not a tensor
        with pytest.raises(ValueError, match="out"):
            sc.render_light_groups(out=out)
    assert sc._native is None  # nothing was uploaded


# ---------------------------------------------------------------- the expectation against the oracle
def test_one_group_of_everything_is_the_oracles_render():
    for name in ("TwoSpheresPlane", "MirrorRefraction"):
        d = bundle(name, (24, 18))
        everything = [list(range(len(d["lights"])))]
        want = LG.expected(d, everything, 0)
        assert want.shape == (1, 18, 24, 3) and want.dtype == np.float32 and not want.flags.writeable
        assert np.array_equal(want[0], LG.to_rows(O.OracleScene(d, LG.ASSETS).render()))
        assert LG.edited(d, range(len(d["lights"])), True) == d


def test_a_removed_light_is_a_black_light():
    """The exactness argument on the oracle itself: the render without a light equals the render
    with that light's colour set to zero (its terms add +0), and a zero ambient equals none."""
    d = bundle("TwoSpheresPlane", (24, 18))
    for li in range(2):
        black = copy.deepcopy(d)
        black["lights"][li]["colour"] = [0, 0, 0]
        removed = LG.edited(d, [k for k in range(2) if k != li], True)
        assert len(removed["lights"]) == 1 and removed["lights"][0] == d["lights"][1 - li]
        a, b = O.OracleScene(removed, LG.ASSETS).render(), O.OracleScene(black, LG.ASSETS).render()
        assert np.array_equal(a, b) and a.any()
    planes = LG.expected(d, [[0], [1]], "own")
    assert planes.shape == (3, 18, 24, 3)
    assert LG.edited(d, [], False)["ambient"] == [0, 0, 0] and LG.edited(d, [], False)["lights"] == []
