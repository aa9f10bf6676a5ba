"""Shadow bins (rtx_api.hip shadow_bins / sb_bin; SceneView::bin_shadow) on the host: the
device source run on the CPU (tests/native/rtx_shadowemu.hip).

Masks hold every ray: for every pixel's level-0 hit point, every light and every sphere and
box, the object alone is tested by the device's own occluded(); wherever it occludes, its bit
must be set in the tile's word. The same check must fail with the table zeroed, and with the
inflation removed (margin 0: no 2-pixel pad, no growth of the occluders, no rho). Random
seeds do not show the latter -- what the margins guard is fp32 rounding of about 1e-6 of
the scene's size -- so those cases are constructed (shadow_scenes.TANGENT_CASES): a sphere
beside the hull edge from a tile's corner ground hit to the light, its radius inside the
~2e-6 window between the fp64 distance to that edge and the radius at which the device's
fp32 shadow ray of the corner pixel already meets it. There the margin-0 table clears a bit
whose test passes, and the product's table (margin 1) holds it.

Seeds (tests/shadow_scenes.py flat_scene, chosen on the CPU): in each of them some object
occludes somewhere and at least a quarter of the tiles clear a bit (asserted below, against a
vacuous pass). seed % 4 picks the kind: 0 plain, 1 camera inside a sphere, 2 one moving sphere, 3 a 15 or 120 degree field of
view; lights are point and directional, below the ground, inside spheres and between the
camera and the objects; spheres and boxes touch the ground."""
import functools

import numpy as np
import pytest

import shadowemu
from common import assert_parity, oracle_render_dict, product_scene_dict
from shadow_scenes import TANGENT_CASES, flat_scene, tangent_scene

SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16]
RES = (96, 72)


@functools.lru_cache(maxsize=None)
def _scene(seed):
    return flat_scene(seed, res=RES)


def _check(sc, subimage=0, tasks=1):
    r = shadowemu.masks(sc, subimage, tasks)
    assert r is not None, "the camera got no shadow bins"
    m = r[0]
    occ, bad, hits = shadowemu.check(sc, m, subimage, tasks)
    assert hits > 0 and occ > 0
    assert bad == 0, "%d of %d occluding tests have their bit clear" % (bad, occ)
    # not vacuous: at least a quarter of the tiles clear at least one (light, object) bit
    every = np.bitwise_or.reduce(m.reshape(-1))
    cleared = float((m != every).any(axis=2).mean())
    assert cleared >= 0.25, cleared
    # sensitivity: an empty table must lose every occluding test
    assert shadowemu.check(sc, np.zeros_like(m), subimage, tasks)[1] == occ
    return m


@pytest.mark.parametrize("seed", SEEDS)
def test_masks_hold_every_ray(seed):
    d = _scene(seed)
    m = _check(product_scene_dict(d))
    assert m.shape == (9, 12, len(d["lights"]))


@pytest.mark.parametrize("strip", [0, 1, 2])
def test_masks_hold_every_ray_in_strips(strip):
    _check(product_scene_dict(_scene(0)), strip, 3)


@pytest.mark.parametrize("seed", SEEDS)
def test_equal_to_the_walk_and_the_oracle(seed):
    d = _scene(seed)
    sc = product_scene_dict(d)
    on, cnt_on, bound = shadowemu.render(sc, True)
    assert bound
    off, cnt_off, bound0 = shadowemu.render(sc, False)
    assert not bound0
    assert np.array_equal(on, off)
    assert np.array_equal(cnt_on, cnt_off)
    assert_parity(on, oracle_render_dict(d), "flat_scene %d" % seed)


@pytest.mark.parametrize("case", range(len(TANGENT_CASES)))
def test_inflation_removed_loses_a_passing_test(case):
    sc = product_scene_dict(tangent_scene(case))
    bare = shadowemu.masks(sc, margin=0.0)[0]
    occ, bad, hits = shadowemu.check(sc, bare)
    assert occ > 0 and bad >= 1, (occ, bad)
    full = shadowemu.masks(sc)[0]
    assert shadowemu.check(sc, full)[1] == 0
    assert (full != np.bitwise_or.reduce(full.reshape(-1))).any()  # (and still clears bits elsewhere)


def test_cameras_and_scenes_without_a_table():
    """Lens cameras, scenes with a mesh and scenes with nothing to occlude get none."""
    d = dict(_scene(0))
    d["AA"] = {"jitter": False, "samples": 2}
    assert shadowemu.masks(product_scene_dict(d)) is None
    d = dict(_scene(0))
    d["objects"] = [o for o in d["objects"] if o["type"] == "plane"]
    assert shadowemu.masks(product_scene_dict(d)) is None
