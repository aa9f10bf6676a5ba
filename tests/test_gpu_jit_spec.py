"""The kernel librtx.so compiles for a scene and camera (option jit_dump prints its name,
options and source) is the one the host emulation's rtx_hostemu_jit_spec describes: both set
the camera up with the same table builder, so tools/jit_offline.py --config compiles what the
library runs. (Frame sizes no other test uses: jit_dump speaks only for a kernel that is not
in memory yet.)"""
import shlex

import pytest

from common import OPTS, product_scene
from jitspec import SCENES, jit_spec

pytestmark = pytest.mark.gpu

SIZES = {"TwoSpheresPlane": (88, 40), "TorusMesh": (56, 48), "MirrorRefraction": (72, 40), "DepthOfField": (40, 24)}


@pytest.mark.parametrize("name,edits,grants", SCENES, ids=[s[0] for s in SCENES])
def test_the_library_compiles_the_offline_spec(name, edits, grants, monkeypatch, capfd):
    monkeypatch.setattr(OPTS, "jit_dump", "1")
    sc = product_scene(name, SIZES[name], **edits)
    kernel, opts, src = jit_spec(sc)
    capfd.readouterr()
    sc.render_device()
    assert sc.jit_wait() == 0
    err = capfd.readouterr().err
    assert sc.last_kernel == kernel, (sc.last_kernel, kernel)
    head = "librtx: jit %s:" % kernel
    at = err.find(head)
    assert at >= 0, "no jit_dump of %s in:\n%s" % (kernel, err[:2000])
    line, _, rest = err[at:].partition("\n")
    no_arch = lambda o: [x for x in o if not x.startswith("--offload-arch=")]
    assert no_arch(shlex.split(line[len(head):])) == no_arch(opts)
    assert rest.startswith(src), "the dumped source differs from the offline spec's"
