"""A ragged strip through the first-hit passes: rows [3, 10) of a 19 x 13 image, so neither the
first row, the row count nor the width is a multiple of the 8 x 8 tile. These are the smallest
inputs at which the lane masking and the tile's bin lookup of the prologue that k_aov and
k_occlusion share can go wrong. Flat, mesh, hierarchy and hierarchy + mesh scenes, without
jitter and with replayed jitter; every comparison is np.array_equal against the host references
of test_gpu_aov.py (the oracle's first hit) and test_gpu_occlusion.py (tests/occref.py)."""
import numpy as np
import pytest

import rtx
from common import product_scene_dict
import occref
import test_gpu_aov as A
import test_gpu_occlusion as OC

pytestmark = pytest.mark.gpu

RES, ROW0, NROWS = (19, 13), 3, 7


def _scene(kind):
    from scenegen import random_hier_scene
    if kind == "flat":
        return A.bundle("TwoSpheresPlane", RES)
    if kind == "mesh":
        return A.bundle("TorusMesh", RES)
    return random_hier_scene(1, res=RES, mesh=kind == "hier+mesh")


@pytest.mark.parametrize("jitter", [False, True], ids=["plain", "replay"])
@pytest.mark.parametrize("kind", ["flat", "mesh", "hier", "hier+mesh"])
def test_ragged_strip_matches_the_host_references(kind, jitter):
    d = _scene(kind)
    d["AA"] = {"jitter": jitter, "samples": 2}
    sc = product_scene_dict(d)
    noise = None
    if jitter:
        noise = np.random.RandomState(5).rand(RES[0] * RES[1] * sc.vc.dof_samples * sc.samples * 3)
        sc.jitter_noise = noise
    rows = slice(ROW0, ROW0 + NROWS)
    # k_aov against the oracle's first hit
    got = A.host(sc.render_aovs(row0=ROW0, nrows=NROWS))
    want = {n: a[rows] for n, a in A.oracle_buffers(d, sc, noise=noise).items()}
    assert got["depth"].shape == (NROWS, RES[0])
    hit = A.check(got, want, kind)
    assert hit.any(), kind
    # k_occlusion against occref, from the hit points and normals just checked
    dirs = rtx.cosine_directions(4)
    occ = OC.host(sc.render_occlusion(ao_samples=4, row0=ROW0, nrows=NROWS))
    want_l, want_a, hit2 = occref.expected(occref.oracle_scene(d, A.ASSETS), sc.lights, got,
                                           float(sc.vc.motion_times[0]), dirs)
    assert np.array_equal(hit, hit2)
    assert np.array_equal(occ["lights"], want_l) and np.array_equal(occ["ao"], want_a), kind
    # the strip is the full pass's rows
    full = OC.host(sc.render_occlusion(ao_samples=4))
    assert np.array_equal(full["lights"][rows], occ["lights"]) and np.array_equal(full["ao"][rows], occ["ao"])
