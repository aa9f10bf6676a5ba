"""Wave-uniform hits (rtx_trace.h cast_ray / shade_uniform<K>) through the host emulation, where
every hit on one of a flat scene's first four objects takes the per-object shading copy (one
lane per wave): frames and ray tallies against the oracle, bit for bit (compared as uint32
words, so NaNs compare). No lighting is skipped anywhere (the unlit skip was measured and left
out): the scenes with unlit, -0.0 and specular-only materials, a negative light
colour and a light on the plane check the copy's literal materials and its select between a
checker plane's two records on values where a wrong word shows -- signs of zero, a differing
spec_zero, NaN. A fifth object falls back to the per-lane path, as do TorusMesh's mesh hits and
all of MirrorRefraction.

Tried once on the host build: shade_uniform<K> wired to object (K + 1) % 3 fails every frame
case here but MirrorRefraction (14 of 15) and six cases of test_hostemu_parity.py's
test_hostemu_bit_exact (TwoSpheresPlane, TorusMesh, MotionBlur, DepthOfField)."""
import numpy as np
import pytest

import hostemu
import uniform_scenes as U
from common import oracle_render_dict, product_scene_dict


def _bits(img):
    return np.ascontiguousarray(np.asarray(img, np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def all_scenes():
    out = {(n, r): d for r in U.RES for n, d in U.scenes(r).items() if r == U.RES[0] or n in ("tsp", "light_on_plane")}
    out[("MirrorRefraction", (64, 36))] = U.bundled("MirrorRefraction", (64, 36))
    out[("TorusMesh", (48, 48))] = U.bundled("TorusMesh", (48, 48))
    return out


NAMES = [(n, U.RES[0]) for n in ("tsp", "both_unlit", "one_material", "zero_diffuse_specular", "negative_zero_diffuse",
                                 "negative_light", "light_on_plane", "directional", "box", "over_cap", "moving")]
NAMES += [("tsp", U.RES[1]), ("light_on_plane", U.RES[1]), ("MirrorRefraction", (64, 36)), ("TorusMesh", (48, 48))]


@pytest.mark.parametrize("name,res", NAMES)
def test_hostemu_frames_and_tallies_equal_the_oracle(all_scenes, name, res):
    d = all_scenes[(name, res)]
    img, cnt = hostemu.render(product_scene_dict(d))
    ref, tl = oracle_render_dict(d, tallies=True)
    assert img.shape == ref.shape
    assert np.array_equal(_bits(img), _bits(ref)), "%s: %d words differ" % (name, int((_bits(img) != _bits(ref)).sum()))
    assert list(cnt[:10]) == tl[:10] and cnt[10] == tl[11] and cnt[11] == tl[12]


@pytest.mark.parametrize("res", U.RES)
def test_tiny_frames_hold_every_tile_class(res):
    """Not vacuous: each tiny TwoSpheresPlane frame has tiles that miss entirely, that hit and
    miss, that see one object and two, all unlit and lit/unlit mixed."""
    cls = U.tile_classes(U.tsp(res))
    assert all(v > 0 for v in cls.values()), cls


def test_light_on_plane_has_a_zero_shadow_direction():
    """The light of `light_on_plane` sits exactly on a black pixel's fp32 hit point."""
    d = U.scenes(U.RES[0])["light_on_plane"]
    sc = product_scene_dict(d)
    o, dr, _ = U.primary_rays(sc)
    p = hostemu.intersect(sc, o, dr)["position"]
    L = np.asarray(d["lights"][1]["position"], np.float32)
    assert (np.abs(p - L).max(axis=1) == 0).any()
