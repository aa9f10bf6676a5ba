"""Tests-only: the scene-specialized render kernel the host emulation says librtx.so builds
for a scene and its camera (tests/native/rtx_hostemu.hip rtx_hostemu_jit_spec, which sets the
camera up with the library's own table builder), and the scenes the two spec tests share."""
import ctypes as C

import hostemu

ONE = {"AA": {"jitter": False, "samples": 1}}
# scene, edits, and which per-camera tables rtx_camera_set grants its kernel:
#   shadow bins   flat scenes of primary and shadow rays, pinhole camera
#   prim origin   one sample, no jitter, static, no secondary rays, no hierarchy
#   tile sched    scenes with secondary rays or a mesh, no hierarchy
SCENES = [
    ("TwoSpheresPlane", ONE, dict(shadow=True, origin=True, sched=False)),
    ("MirrorRefraction", ONE, dict(shadow=False, origin=False, sched=True)),
    ("TorusMesh", ONE, dict(shadow=False, origin=True, sched=True)),
    ("DepthOfField", {}, dict(shadow=False, origin=False, sched=False)),
]
MACROS = {"shadow": "-DRTX_SHADOW_BINS=1", "origin": "-DRTX_PRIM_ORIGIN=1", "sched": "-DRTX_TILE_SCHED=1"}


def jit_spec(scene, counters=False, rgb8=False):
    """(kernel name, hiprtc options, source) of the scene's render kernel, or None when the
    generic kernel runs."""
    sd = scene.scene_desc()
    cd, tables = scene.camera_desc()
    f = hostemu.lib().rtx_hostemu_jit_spec
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
    f.restype = C.c_int64
    args = (C.addressof(sd), C.addressof(cd), 1 if counters else 0, 1 if rgb8 else 0)
    n = f(*args, None, 0)
    if n == -1:
        return None
    assert n > 0, hostemu.lib().rtx_hostemu_last_error().decode()
    buf = C.create_string_buffer(int(n) + 1)
    f(*args, buf, n + 1)
    head, src = buf.value.decode().split("\n\n", 1)
    name, *opts = head.split("\n")
    return name, opts, src
