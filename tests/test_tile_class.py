"""Tile classes (rtx_api.hip sb_bin / tile_classes; SceneView::bin_class; option tile_class) on
the host: the device source run on the CPU (tests/native/rtx_classemu.hip).

Soundness: every flag of every bin is checked at every pixel of the bin by the device's own
tests with nothing culled -- a SKY pixel's closest_hit misses, a PLANE pixel's hit is object
0, and from an UNSHADOWED pixel's hit point occluded() of the whole scene (the plane's own test
included) is false for every light. The check is shown to fail: on forged records, and on the
records built without the margins (margin 0) for the constructed scenes whose sphere lies
within fp32 rounding of a tile's shadow hull (shadow_scenes.TANGENT_CASES).

Same frame: the emulated render that reads the records equals the one without them (option
tile_class 0), image and tallies, for whole frames, a row block off the 8-row grid and
interleaved groups."""
import copy
import functools

import numpy as np
import pytest

import classemu
from classemu import PLANE, SKY, UNSHADOWED
from class_scenes import CAM, EDGE_AT, LOOK, constructed, scene_dict, sphere
from common import product_scene, product_scene_dict
from shadow_scenes import TANGENT_CASES, flat_scene, tangent_scene

SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16]
SIZES = [(72, 40), (61, 35)]
ONE = {"AA": {"jitter": False, "samples": 1}}


@functools.lru_cache(maxsize=None)
def _seeded(seed, res):
    return flat_scene(seed, res=res)


def _one_time(d):
    """d with its motion blur reduced to one motion time (a camera the records are built for)."""
    e = copy.deepcopy(d)
    if "motion" in e:
        e["motion"] = {"time": e["motion"]["time"], "samples": 1, "final": 0}
    return e


def _sound(sc, subimage=0, tasks=1, rec=None):
    """The camera's records, every flag checked at every pixel."""
    if rec is None:
        rec = classemu.records(sc, subimage, tasks)
    assert rec is not None, "the camera got no class records"
    r = classemu.check(sc, rec, subimage, tasks)
    print("classes: sky %s plane %s unshadowed %s" % (r["sky"], r["plane"], r["unshadowed"]))
    assert r["sky"][1] == 0, "%d of %d SKY pixels hit something" % (r["sky"][1], r["sky"][0])
    assert r["plane"][1] == 0, "%d of %d PLANE pixels do not hit the plane" % (r["plane"][1], r["plane"][0])
    assert r["unshadowed"][1] == 0, "%d of %d UNSHADOWED shadow tests are occluded" % (r["unshadowed"][1], r["unshadowed"][0])
    cls = rec[:, :, 1]
    assert not ((cls & UNSHADOWED) != 0)[(cls & PLANE) == 0].any()  # UNSHADOWED only with PLANE
    assert not ((cls & SKY) != 0)[(cls & PLANE) != 0].any()
    assert not (cls != 0)[rec[:, :, 0] != 0].any()  # no flag where an object may be hit
    return rec, r


# ---------------------------------------------------------------- soundness per pixel
@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("seed", SEEDS)
def test_flags_hold_at_every_pixel(seed, res):
    d = _seeded(seed, res)
    sc = product_scene_dict(d)
    if "motion" in d:  # two motion times: no one-sample kernel, no records; its one-time copy gets them
        assert classemu.records(sc) is None
        sc = product_scene_dict(_one_time(d))
    rec, _ = _sound(sc)
    assert rec.shape == ((res[1] + 7) // 8, (res[0] + 7) // 8, 2)
    # the record's mask is the bins' own
    import hostemu
    assert np.array_equal(rec[:, :, 0], hostemu.bins(sc)[0])
    # and the camera's own table holds the same records
    assert np.array_equal(classemu.bound(sc), rec)


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("strip", [0, 1, 2])
def test_flags_hold_in_strips(strip, res):
    _sound(product_scene_dict(_seeded(0, res)), strip, 3)


@pytest.mark.parametrize("res", SIZES)
def test_two_spheres_plane(res):
    assert classemu.records(product_scene("TwoSpheresPlane", res)) is None  # as bundled: several samples per pixel
    rec, r = _sound(product_scene("TwoSpheresPlane", res, **ONE))
    assert r["unshadowed"][0] > 0 and r["plane"][0] > r["unshadowed"][0] // 2  # (two lights' tests per pixel)


def test_forged_records_fail_the_check():
    """The check can fail: with every bin forged SKY, PLANE or UNSHADOWED it reports pixels."""
    sc = product_scene("TwoSpheresPlane", (72, 40), **ONE)
    rec = classemu.records(sc)
    for flag, key in ((SKY, "sky"), (PLANE, "plane"), (PLANE | UNSHADOWED, "unshadowed")):
        forged = rec.copy()
        forged[:, :, 1] = flag
        assert classemu.check(sc, forged)[key][1] > 0, key


# ---------------------------------------------------------------- the same frame
def _frames_equal(sc, H):
    try:
        classemu.set_option("tile_class", "1")
        assert classemu.bound(sc) is not None
        on, cnt_on = classemu.render(sc)
        blk_on, bcnt_on = classemu.render_block(sc, 3, H - 5)
        rows = [r for g in range(1, (H + 7) // 8, 2) for r in range(8 * g, min(8 * g + 8, H))]
        grp_on = classemu.render_rows(sc, rows)
        classemu.set_option("tile_class", "0")
        assert classemu.bound(sc) is None
        off, cnt_off = classemu.render(sc)
        blk_off, bcnt_off = classemu.render_block(sc, 3, H - 5)
        grp_off = classemu.render_rows(sc, rows)
    finally:
        classemu.set_option("tile_class", "1")
    for a, b in ((on, off), (blk_on, blk_off), (grp_on, grp_off)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(cnt_on, cnt_off), (cnt_on, cnt_off)
    assert np.array_equal(bcnt_on, bcnt_off), (bcnt_on, bcnt_off)
    assert np.array_equal(blk_on.view(np.uint32), on[3:H - 2].view(np.uint32))
    assert np.array_equal(grp_on.view(np.uint32), on[rows].view(np.uint32))


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("seed", SEEDS)
def test_same_frame_on_and_off(seed, res):
    _frames_equal(product_scene_dict(_one_time(_seeded(seed, res))), res[1])


@pytest.mark.parametrize("res", SIZES)
def test_same_frame_two_spheres_plane(res):
    _frames_equal(product_scene("TwoSpheresPlane", res, **ONE), res[1])


# ---------------------------------------------------------------- constructed cameras
def _classes(d, frames=True):
    sc = product_scene_dict(d)
    rec, r = _sound(sc)
    if frames:
        _frames_equal(sc, d["resolution"][1])
    return rec[:, :, 1], r


@pytest.mark.parametrize("res", SIZES)
def test_camera_looking_away_from_the_plane(res):
    """Above the plane looking up, and under it looking down: every tile is SKY. Under it looking
    up, every ray meets the plane from below."""
    sc = constructed(res)
    for name in ("sky_above", "sky_below"):
        cls, _ = _classes(sc[name])
        assert (cls == SKY).all(), (name, cls)
    cls, _ = _classes(sc["plane_from_below"])
    assert ((cls & PLANE) != 0).all(), cls


@pytest.mark.parametrize("res", SIZES)
def test_horizon_through_a_tile_row(res):
    """A level camera: the horizon runs through the middle rows, whose tiles get no flag (nor
    do those within the bins' 2-pixel pad of it); SKY above, PLANE below."""
    cls, _ = _classes(constructed(res)["horizon"])
    hrow = (res[1] // 2) // 8  # the tile row of the image's middle rows
    assert (cls[hrow] == 0).all(), cls
    assert (cls[0] == SKY).all() and ((cls[-1] & PLANE) != 0).all(), cls
    for row in cls[:hrow]:
        assert (row == SKY).all() or (row == 0).all(), cls
    for row in cls[hrow + 1:]:
        assert ((row & PLANE) != 0).all() or (row == 0).all(), cls


def _edge(rad):
    return scene_dict(CAM, LOOK, [sphere(EDGE_AT, rad)])


@pytest.mark.parametrize("rad", [round(0.60 + 0.01 * i, 2) for i in range(12)])
def test_sphere_at_a_tile_edge(rad):
    """A sphere whose silhouette grows across tile borders: every flag holds at every radius."""
    cls, r = _classes(_edge(rad), frames=(rad in (0.6, 0.71)))
    assert (cls == 0).any() and (cls != 0).any()


def test_sphere_at_a_tile_edge_moves_the_border():
    """Over those radii some tile beside the sphere turns from a class to none."""
    n = [int((_classes(_edge(rad), frames=False)[0] != 0).sum()) for rad in (0.60, 0.71)]
    assert n[1] < n[0], n


@pytest.mark.parametrize("case", range(len(TANGENT_CASES)))
def test_shadow_just_reaching_a_tile(case):
    """The sphere's shadow hull touches a tile's corner hit within fp32 rounding: the product's
    records hold; without the margins that tile is UNSHADOWED and the check reports it."""
    sc = product_scene_dict(tangent_scene(case))
    rec, r = _sound(sc)
    assert r["unshadowed"][0] > 0
    bare = classemu.records(sc, margin=0.0)
    bad = classemu.check(sc, bare)
    print("margin 0:", bad)
    assert bad["unshadowed"][1] >= 1, bad
    assert ((bare[:, :, 1] & UNSHADOWED) != 0).sum() > ((rec[:, :, 1] & UNSHADOWED) != 0).sum()


def test_plane_self_limit_inside_the_frame():
    """A light 2 above the plane: its plane_self limit lies inside the frame, so near tiles are
    UNSHADOWED and far ones PLANE alone; without the growth by rho the bound only shrinks."""
    import hostemu
    d = constructed()["plane_self_inside"]
    sc = product_scene_dict(d)
    lim = float(hostemu.plane_self(sc)[0, 0])
    assert 2.0 < lim < 30.0, lim
    cls, r = _classes(d)
    assert (cls == (PLANE | UNSHADOWED)).any() and (cls == PLANE).any(), cls
    bare = classemu.records(sc, cls_rho=0.0)[:, :, 1]
    assert not ((cls & UNSHADOWED) != 0)[(bare & UNSHADOWED) == 0].any()


def test_plane_self_limit_of_minus_one():
    """A light 0.1 above the plane: no limit (-1), so the plane's own test always runs and no tile
    is UNSHADOWED."""
    import hostemu
    d = constructed()["plane_self_none"]
    assert float(hostemu.plane_self(product_scene_dict(d))[0, 0]) == -1.0
    cls, _ = _classes(d)
    assert ((cls & PLANE) != 0).any() and not ((cls & UNSHADOWED) != 0).any(), cls


def test_two_planes_get_no_plane_flag():
    cls, _ = _classes(constructed()["two_planes"])
    assert not ((cls & PLANE) != 0).any(), cls


def test_directional_light():
    """A directional light's plane_self limit is small (0.17 here: no term of it grows with the
    light's distance), so its tiles stay PLANE alone; every flag holds."""
    cls, r = _classes(constructed()["directional"])
    assert (cls == PLANE).any() and not ((cls & UNSHADOWED) != 0).any(), cls


def test_seventeen_spheres():
    """The 17th sphere is always tested: its bit stays set in every word, so no tile is UNSHADOWED."""
    cls, _ = _classes(constructed()["seventeen"])
    assert not ((cls & UNSHADOWED) != 0).any(), cls


def test_moving_sphere():
    """A moving sphere is always tested: no tile is UNSHADOWED; SKY and PLANE tiles remain."""
    cls, _ = _classes(constructed()["moving"])
    assert not ((cls & UNSHADOWED) != 0).any() and (cls != 0).any(), cls
    sc = product_scene_dict(constructed()["moving"])
    sc.vc.motion_times = [0.7]  # (away from its rest position: the bins hold its sweep)
    rec, _ = _sound(sc)
    assert not ((rec[:, :, 1] & UNSHADOWED) != 0).any()
    _frames_equal(sc, 40)


# ---------------------------------------------------------------- the classifier fires
def test_the_classifier_fires_at_1080p():
    """Bundled TwoSpheresPlane at 1920x1080, tables only: SKY or UNSHADOWED tiles number at least
    half of the 25,281 tiles whose object mask and shadow words are empty (a floor a classifier
    that never fires cannot meet, not a target)."""
    rec = classemu.records(product_scene("TwoSpheresPlane", (1920, 1080), **ONE))
    cls = rec[:, :, 1]
    counts = {"tiles": int(cls.size), "sky": int((cls == SKY).sum()), "plane only": int((cls == PLANE).sum()),
              "unshadowed": int((cls == (PLANE | UNSHADOWED)).sum()), "none": int((cls == 0).sum())}
    print(counts)
    assert counts["tiles"] == 32400
    assert counts["sky"] + counts["unshadowed"] >= 12641, counts
