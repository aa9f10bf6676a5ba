"""The offline kernel spec (rtx_hostemu_jit_spec; tools/jit_offline.py --config) carries the
options of the per-camera tables: its camera is set up by the builder rtx_camera_set uses
(rtx_api.hip CamTables), so the primary bins and, where the product's predicates grant them,
the shadow bins, the primary rays' origin terms and the tile schedule are compiled in."""
import pytest

from common import product_scene
from jitspec import MACROS, SCENES, jit_spec


@pytest.mark.parametrize("name,edits,grants", SCENES, ids=[s[0] for s in SCENES])
def test_spec_carries_the_camera_tables(name, edits, grants):
    spec = jit_spec(product_scene(name, (64, 48), **edits))
    assert spec is not None
    kernel, opts, src = spec
    assert kernel.startswith("rtx_jit_render_") and kernel in src
    assert "-DRTX_PRIMARY_BINS=1" in opts
    for key, macro in MACROS.items():
        assert (macro in opts) == grants[key], (name, macro, opts)
