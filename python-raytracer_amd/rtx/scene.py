"""Scene: the reference's render entry point, running on MI355X through librtx.so.

Mirror of provided/scene.py:16-209. ``Scene.render(subimage=0, tasks=1)`` keeps the
reference's signature and result: a float64 array of shape (strip_width, height, 3),
indexed [column, row-from-bottom, rgb], where the strip is
``np.array_split(np.arange(width), tasks)[subimage]`` (scene.py:36-37). The per-pixel
loops, cast_ray, shading and the intersectors run in HIP kernels (csrc/); this module
only prepares the reference's scalar tables (pixel x/y running sums, sunflower origins,
motion times) and moves buffers.
"""
import ctypes as C
import hashlib
import itertools
import math

import numpy as np
import torch

from . import _native as N
from . import f32 as F
from . import records
from . import track
from .helperclasses import sunflower, sunflower_many

DEFAULT_SEED = 0x5EED
# the first-hit feature buffers of Scene.render_aovs (rtx_render_aov)
AOV_NAMES = ("depth", "normal", "position", "albedo", "object", "material")
_AOV_VEC = ("normal", "position", "albedo")
_AOV_INT = ("object", "material")
# the occlusion buffers of Scene.render_occlusion (rtx_render_occlusion)
OCCLUSION_NAMES = ("lights", "ao")
# the all-sample buffers of Scene.render_resolved (rtx_render_resolved), in the entry's order
RESOLVED_NAMES = ("alpha", "matte", "depth", "normal", "albedo")
_RESOLVED_VEC = ("normal", "albedo")
# the ranked id-coverage buffers of Scene.render_ids (rtx_render_ids), in the entry's order
ID_NAMES = ("ids", "counts", "other")
_ID_KEYS = {"object": N.RTX_ID_OBJECT, "material": N.RTX_ID_MATERIAL}


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def running_sum(x0, dx, n):
    """[x0, x0 + dx, (x0 + dx) + dx, ...] (n values) in fp64, each step one rounded add --
    the reference's `x += dx` loop (scene.py:39-45); ufunc accumulate adds in order."""
    if n <= 0:
        return np.empty(0, np.float64)
    steps = np.full(n, dx, np.float64)
    steps[0] = x0
    return np.add.accumulate(steps)


def strip_columns(width, subimage, tasks):
    """np.array_split(np.arange(width), tasks)[subimage] as (first column, count)."""
    if tasks < 1 or not 0 <= subimage < tasks:
        raise IndexError("subimage %d out of range for %d tasks" % (subimage, tasks))
    base, extra = divmod(width, tasks)
    col0 = subimage * base + min(subimage, extra)
    n = base + (1 if subimage < extra else 0)
    if n == 0:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")  # width[0] on an empty strip
    return col0, n


def split_rows(height, n, k):
    """np.array_split(np.arange(height), n)[k] as (first row, count): rank k's row block."""
    base, extra = divmod(height, n)
    return k * base + min(k, extra), base + (1 if k < extra else 0)


def group_rows(height, n, k):
    """Image rows (row 0 = top) of rank k's interleaved 8-row groups k, k + n, ... (the
    rows rtx_render_groups packs, in order), as an int64 array."""
    g = np.arange(k, (height + 7) // 8, n)
    rows = (g[:, None] * 8 + np.arange(8)[None, :]).ravel()
    return rows[rows < height]


def fb_to_rgb8(fb, out=None, stream=None):
    """rtx_fb_to_rgb8 on the device: (fb * 255.0) truncated to uint8 (main.py:33), into
    ``out`` (a contiguous uint8 CUDA tensor of fb's shape) or a new tensor."""
    if not (fb.is_cuda and fb.dtype == torch.float32 and fb.is_contiguous()):
        raise ValueError("fb must be a contiguous float32 CUDA tensor")
    if out is None:
        out = torch.empty(fb.shape, dtype=torch.uint8, device=fb.device)
    if out.shape != fb.shape or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 CUDA tensor of shape %s" % (tuple(fb.shape),))
    st = stream if stream is not None else torch.cuda.current_stream()
    N.call("rtx_fb_to_rgb8", C.c_void_p(fb.data_ptr()), C.c_void_p(out.data_ptr()), int(fb.numel()),
           C.c_void_p(st.cuda_stream))
    return out


def frame_windows(start, stop, frames, shutter=0.0, samples=1, final=0):
    """The motion-time windows of ``frames`` frames over [start, stop), for
    Scene.render_sequence: frame f opens at t_f = start + (stop - start) / frames * f, and
    its window is ViewportCamera.set_motion's rule shifted to t_f --
    [t_f + shutter / samples * i for i in range(samples)] + [t_f + shutter] * final
    (shutter 0.0, samples 1: the single time t_f). Python float arithmetic throughout."""
    frames, samples, final = int(frames), int(samples), int(final)
    if frames < 1 or samples < 0 or final < 0 or samples + final < 1:
        raise ValueError("frame_windows needs frames >= 1 and samples + final >= 1 (none negative)")
    start, stop, shutter = float(start), float(stop), float(shutter)
    step = (stop - start) / frames
    dt = shutter / samples if samples else 0.0
    out = []
    for f in range(frames):
        t = start + step * f
        out.append([t + dt * i for i in range(samples)] + [t + shutter] * final)
    return sequence_windows(out)


def sequence_windows(windows):
    """``windows`` as a list of F >= 1 lists of T >= 1 Python floats (a flat sequence of
    numbers: T = 1). ValueError for an empty, ragged or non-finite sequence."""
    try:
        rows = list(windows)
        if rows and all(np.ndim(w) == 0 for w in rows):
            rows = [[w] for w in rows]
        rows = [[float(t) for t in w] for w in rows]
    except TypeError:
        raise ValueError("windows must be a sequence of equal-length sequences of motion times") from None
    if not rows or not rows[0]:
        raise ValueError("a frame sequence needs at least one window of at least one motion time")
    if any(len(w) != len(rows[0]) for w in rows):
        raise ValueError("every window of a frame sequence holds the same number of motion times")
    if not all(math.isfinite(t) for w in rows for t in w):
        raise ValueError("motion times must be finite")
    return rows


# ---- argument checks the render methods share
def _buffer_names(method, a_noun, known, names):
    """The buffers asked of ``method`` as a list: each one of ``known``, none twice. ``a_noun``
    names such a buffer in the messages, with its article ("a feature buffer")."""
    names = [names] if isinstance(names, str) else list(names)
    if not names:
        raise ValueError("%s needs at least one of %s" % (method, known))
    for n in names:
        if n not in known:
            raise ValueError("unknown %s %r (known: %s)" % (a_noun.split(" ", 1)[1], n, ", ".join(known)))
    if len(set(names)) != len(names):
        raise ValueError("%s is named twice: %s" % (a_noun, names))
    return names


def _window_frame(windows, frame):
    """(sequence_windows(windows) or None, frame), the frame inside the windows."""
    if windows is not None:
        windows = sequence_windows(windows)
    frame, n = int(frame), 1 if windows is None else len(windows)
    if not 0 <= frame < n:
        raise ValueError("frame %d outside the %d window(s)" % (frame, n))
    return windows, frame


def _row_range(H, row0, nrows):
    """(row0, nrows) as ints inside an image of H rows; nrows None: down to the last row."""
    row0 = int(row0)
    nrows = H - row0 if nrows is None else int(nrows)
    if row0 < 0 or nrows < 0 or row0 + nrows > H:
        raise ValueError("rows [%d, %d) outside the image of %d rows" % (row0, row0 + nrows, H))
    return row0, nrows


def _out_dict(out, names, table):
    """A copy of the caller's ``out`` dict, its tensors checked against table[name] = (shape, dtype)."""
    out = {} if out is None else dict(out)
    for n in out:
        if n not in names:
            raise ValueError("out holds %r, which is not among the requested buffers %s" % (n, names))
    for n in names:
        shape, dtype = table[n]
        t = out.get(n)
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype
                              or not t.is_cuda or not t.is_contiguous()):
            raise ValueError("out[%r] must be a contiguous %s CUDA tensor of shape %s"
                             % (n, str(dtype).replace("torch.", ""), shape))
    return out


def _out_alloc(out, names, table):
    """The requested buffers, in order: the caller's where given, new tensors otherwise."""
    for n in names:
        if out.get(n) is None:
            out[n] = torch.empty(table[n][0], dtype=table[n][1], device="cuda")
    return {n: out[n] for n in names}


def id_matte(ids, counts, members, samples):
    """The matte of the keys ``members`` out of Scene.render_ids' buffers: float32 [nrows, W],
    fl32(the sum of ``counts`` where ``ids`` is in ``members``) / fl32(``samples``), in torch on the
    tensors' device. It has the meaning of render_resolved's "matte" and equals it bit for bit
    where "other" is 0 (every hit of the pixel is then in a written rank). ``ids`` and ``counts``:
    int32 [nrows, W, ranks]; ``members``: a non-empty sequence of object or material indices;
    ``samples``: the camera's samples per pixel (Scene.samples_per_pixel)."""
    for name, t in (("ids", ids), ("counts", counts)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 3:
            raise ValueError("%s must be an int32 tensor of shape [nrows, W, ranks]" % name)
    if ids.shape != counts.shape or ids.device != counts.device:
        raise ValueError("ids and counts must have one shape and one device")
    try:
        keys = [m for m in members]
    except TypeError:
        raise ValueError("members must be a sequence of indices") from None
    if not keys or any(isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 0 for m in keys):
        raise ValueError("members must be a non-empty sequence of indices >= 0")
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError("samples must be an integer >= 1, got %r" % (samples,))
    keys = torch.tensor(sorted(set(int(m) for m in keys)), dtype=torch.int32, device=ids.device)
    inside = (ids.unsqueeze(-1) == keys).any(dim=-1)
    n = torch.where(inside, counts, torch.zeros_like(counts)).sum(dim=-1, dtype=torch.int32)
    return n.to(torch.float32) / torch.tensor(float(samples), dtype=torch.float32, device=ids.device)


def light_group_table(n_lights, groups=None, ambient="own"):
    """The arguments of Scene.render_light_groups as rtx_render_light_groups takes them:
    (light_group, n_groups, ambient_group), with light_group an int32 array of ``n_lights``
    entries -- light li's group, or -1 for a light in no group, which lights nothing.

    ``groups``: a sequence of sequences of light indices, group g = groups[g] (a group may be
    empty); None: one group per light, in light order. ``ambient``: "own" (a group of its own,
    appended last), the index of one of ``groups``, or None (the ambient term is dropped).
    ValueError for a light index out of range, a light in two groups, an ambient that is none
    of the three, or more than 8 groups once the ambient's is counted (and for none at all)."""
    n_lights = int(n_lights)
    if groups is None:
        groups = [[li] for li in range(n_lights)]
    try:
        groups = [list(g) for g in groups]
    except TypeError:
        raise ValueError("groups must be a sequence of sequences of light indices") from None
    table = np.full(n_lights, -1, np.int32)
    for g, members in enumerate(groups):
        for li in members:
            if isinstance(li, bool) or not isinstance(li, (int, np.integer)) or not 0 <= li < n_lights:
                raise ValueError("light %r of group %d outside the scene's %d lights" % (li, g, n_lights))
            if table[li] >= 0:
                raise ValueError("light %d is in two groups: %d and %d" % (li, table[li], g))
            table[li] = g
    n_groups = len(groups)
    if ambient is None:
        ambient_group = -1
    elif isinstance(ambient, str):
        if ambient != "own":
            raise ValueError('ambient must be "own", a group index or None, got %r' % (ambient,))
        ambient_group = n_groups
        n_groups += 1
    elif isinstance(ambient, bool) or not isinstance(ambient, (int, np.integer)):
        raise ValueError('ambient must be "own", a group index or None, got %r' % (ambient,))
    elif not 0 <= ambient < n_groups:
        raise ValueError("ambient group %d outside the %d groups" % (ambient, n_groups))
    else:
        ambient_group = int(ambient)
    if not 1 <= n_groups <= N.RTX_LIGHT_GROUPS_MAX:
        raise ValueError("a light-group pass holds 1 to %d groups (the ambient's own included), got %d"
                         % (N.RTX_LIGHT_GROUPS_MAX, n_groups))
    return table, n_groups, ambient_group


def _strip_rows(H, row0, nrows, groups):
    """The row count of a render: of ``groups=(k, n)`` when given, else nrows (None: the rest)."""
    if groups is not None:
        k, n = groups
        nrows = int(N.load().rtx_group_rows(H, int(k), int(n)))
        if nrows < 0:
            raise ValueError("groups=(k, n) needs 0 <= k < n")
    return H - row0 if nrows is None else nrows


def _check_fb(out, shape_ok, shape_text):
    if not shape_ok or out.dtype not in (torch.float32, torch.uint8) or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 or uint8 CUDA tensor " + shape_text)


def _counters_ptr(counters):
    if counters is not None and (counters.numel() < N.RTX_COUNTERS or counters.dtype != torch.int64
                                 or not counters.is_cuda):
        raise ValueError("counters must be an int64 CUDA tensor with >= %d entries" % N.RTX_COUNTERS)
    return C.c_void_p(counters.data_ptr() if counters is not None else 0)


def panorama_rays(vc, width, height):
    """An equirectangular panorama about the camera position, a camera the reference lacks,
    as rays for Scene.cast_rays: (origins, directions), numpy float32 [height * width, 3],
    row 0 at the top, pixel-major. Pixel (r, c) looks along
    d = sin(theta) (cos(phi) (-w) + sin(phi) u) + cos(theta) v with theta = pi (r + 0.5) / height
    and phi = 2 pi (c + 0.5) / width - pi: the image centre looks where the camera does, its
    top along the camera's up. Evaluated in fp64 from the camera's u, v, w and rounded once to
    fp32; the origin is the fp32 camera position."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("a panorama needs width >= 1 and height >= 1")
    u, v, w = (np.asarray(x, np.float32).astype(np.float64).reshape(3) for x in (vc.u, vc.v, vc.w))
    theta = (math.pi * (np.arange(height, dtype=np.float64) + 0.5) / height)[:, None, None]
    phi = (2.0 * math.pi * (np.arange(width, dtype=np.float64) + 0.5) / width - math.pi)[None, :, None]
    d = np.sin(theta) * (np.cos(phi) * -w + np.sin(phi) * u) + np.cos(theta) * v
    o = np.broadcast_to(np.asarray(vc.position, np.float32).reshape(3), d.shape)
    return np.ascontiguousarray(o).reshape(-1, 3), d.astype(np.float32).reshape(-1, 3)


def cosine_directions(k):
    """The default ambient-occlusion directions of Scene.render_occlusion: ``k`` cosine-weighted
    directions about +z (Malley's method), float32 [k, 3]. (x, y) are the sunflower points of
    the unit disk (Scene._sunflower_spread's radii and angles, scene.py:118-138) in fp64,
    z = sqrt(max(0, 1 - x^2 - y^2)); the three are rounded to fp32 once. The outermost point
    lies on the disk's rim, so the last direction runs along the surface (z is 0 or a rounding
    residue)."""
    from .helperclasses import _sunflower_terms
    k = int(k)
    if k < 1:
        raise ValueError("cosine_directions needs k >= 1")
    sq, co, si, sn = _sunflower_terms(k)
    r = sq / sn
    x, y = r * co, r * si
    z = np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y))
    return np.stack([x, y, z], axis=1).astype(np.float32)


_GENERATION = itertools.count(1)


class _NativeScene:
    """Owns an rtx_scene handle (device buffers live until destroy)."""

    def __init__(self, desc):
        h = C.c_void_p()
        N.call("rtx_scene_create", C.byref(desc), C.byref(h))
        self.h = h
        self.device = torch.cuda.current_device()

    def close(self):
        if self.h is not None and self.h.value:
            N.load().rtx_scene_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    # the attributes whose values the uploaded records are made of (with the objects,
    # materials and lights they hold): assigning one counts the edit epoch up (rtx.track)
    _RECORDS = ("objects", "materials", "lights", "ambient")

    def __init__(self, vc, jitter, samples, ambient, lights, materials, objects):
        self.vc = vc
        self.jitter = jitter
        self.samples = samples
        self.ambient = F.vec3(ambient)
        self.lights = lights
        self.materials = materials
        self.objects = objects
        self.seed = DEFAULT_SEED      # Philox key for jitter (the reference's RNG is unseeded)
        self.jitter_noise = None      # optional replayed np.random.rand() stream (parity mode)
        self._native = None
        self._cam_key = None
        self._gen = next(_GENERATION)  # upload generation: new on every re-create / camera upload
        self._digest = None            # digest of the uploaded descriptor's bytes
        self._epoch = -1               # rtx.track epoch at the last check against the upload
        self._tracked = False          # every record reports its edits (rtx.track.scene_tracked)

    def __setattr__(self, name, value):
        if name in self._RECORDS:
            if isinstance(value, np.ndarray) and not isinstance(value, track.TArray):
                value = value.view(track.TArray)
            object.__setattr__(self, name, value)
            track.bump()
            return
        object.__setattr__(self, name, value)

    @classmethod
    def from_reference(cls, ref):
        """Bind a scene built by the reference's own scene_parser.load_scene
        (provided/scene.py:18-33): the same vc / jitter / samples / ambient / lights /
        materials / objects, read through the reference's attribute names (rtx.records)."""
        return cls(ref.vc, ref.jitter, ref.samples, ref.ambient, ref.lights, ref.materials, ref.objects)

    def invalidate(self):
        """Drop the uploaded scene and camera: the next render re-reads every object,
        material, light and camera attribute (the reference reads them on every call)."""
        if self._native is not None:
            self._native.close()
        self._native = None
        self._cam_key = None
        self._noise_src = None
        self._gen = next(_GENERATION)

    @property
    def last_kernel(self):
        """Name of the kernel the last render launched (rtx_last_kernel): a
        scene-specialized "rtx_jit_render_*" or a generic "k_render*"."""
        if self._native is None or not self._native.h:
            return ""
        return N.load().rtx_last_kernel(self._native.h).decode()

    def jit_wait(self, block=True):
        """rtx_jit_wait: the scene-specialized kernels compile on a host thread (option
        jit_async) while the generic kernel renders the same bytes; this picks up finished
        compiles -- block=True: waits for them first -- and returns how many are still
        compiling. Call it before timing frames or capturing them into a graph."""
        if self._native is None or not self._native.h:
            return 0
        n = N.load().rtx_jit_wait(self._native.h, 1 if block else 0)
        if n < 0:
            N.check("rtx_jit_wait", n)
        return n

    # ------------------------------------------------------------------ scene upload
    def scene_desc(self):
        """Flatten the objects into the rtx_scene_desc ABI arrays (scene order kept;
        rtx.records reads the reference's attribute names, so the objects may be the
        reference's own)."""
        return records.scene_desc(self.objects, self.materials, self.lights, self.ambient)

    def native(self):
        """The uploaded scene (rtx_scene_create), kept current with the description: the
        reference reads every object, material and light on every render
        (provided/scene.py:86-88, :148, :161-164), so an edit since the upload re-uploads
        the scene. A scene whose records all report their edits (this package's parser and
        classes, rtx.track) is checked with one epoch compare and flattened again only after
        some edit; other scenes (the reference's own objects, Scene.from_reference) are
        flattened and compared on every call. Either way the upload is redone only when the
        descriptor's bytes differ."""
        dev = torch.cuda.current_device()
        nat = self._native
        if nat is not None and nat.device == dev and self._tracked and track.epoch() == self._epoch:
            return nat
        ep = track.epoch()
        desc = self.scene_desc()
        digest = records.desc_digest(desc)
        if nat is None or nat.device != dev or digest != self._digest:
            self._native = _NativeScene(desc)
            self._cam_key = None
            self._gen = next(_GENERATION)
            self._digest = digest
        self._epoch = ep
        self._tracked = track.scene_tracked(self.objects, self.materials, self.lights, self.ambient)
        return self._native

    # ------------------------------------------------------------------ camera tables
    def camera_tables(self, subimage=0, tasks=1, windows=None):
        """The reference's per-frame scalars (scene.py:36-45, :48-61), evaluated on the host.
        ``windows`` (a frame sequence, sequence_windows): the motion times are its F windows
        of T times, [F][T] flattened, in place of vc.motion_times."""
        vc = self.vc
        col0, ncols = strip_columns(vc.width, subimage, tasks)
        dx = (vc.right - vc.left) / vc.width
        dy = (vc.top - vc.bottom) / vc.height
        # the running sums x += dx, y += dy (scene.py:39-45), in order: add.accumulate
        # adds left to right in fp64, one rounding per step, as the reference's loop does
        xs = running_sum(vc.left + (0.5 + np.int64(col0)) * dx, dx, ncols)
        ys = running_sum(vc.bottom + 0.5 * dy, dy, vc.height)
        dof = sunflower(vc.dof_samples, vc.position, vc.aperture)
        aa = sunflower_many(self.samples, dof, 2 * (dx + dy))
        return dict(col0=col0, ncols=ncols, xs=xs.astype(np.float32), ys=ys.astype(np.float32),
                    dof=np.ascontiguousarray(dof), aa=np.ascontiguousarray(aa),
                    times=np.asarray(vc.motion_times if windows is None else windows, np.float64).ravel(),
                    n_times=len(vc.motion_times) if windows is None else len(windows[0]),
                    n_frames=0 if windows is None else len(windows), jscale=0.1 * (dx + dy))

    def camera_desc(self, subimage=0, tasks=1, windows=None):
        """rtx_camera_desc for the strip; returns (desc, tables). The tables own the
        memory the descriptor points at: keep them alive while the descriptor is used.
        ``windows``: a frame sequence's camera (n_frames windows of n_times motion times)."""
        if windows is not None:
            windows = sequence_windows(windows)
        t = self.camera_tables(subimage, tasks, windows)
        vc = self.vc
        d = N.rtx_camera_desc()
        d.width, d.height, d.col0, d.ncols = vc.width, vc.height, t["col0"], t["ncols"]
        d.xs, d.ys = _ptr(t["xs"], C.c_float), _ptr(t["ys"], C.c_float)
        d.position, d.u, d.v, d.w = N.f3(vc.position), N.f3(vc.u), N.f3(vc.v), N.f3(vc.w)
        d.d, d.focal_length = float(vc.d), float(vc.focal_length)
        d.n_dof, d.n_aa = vc.dof_samples, self.samples
        d.dof_origins, d.aa_origins = _ptr(t["dof"], C.c_float), _ptr(t["aa"], C.c_float)
        d.n_times, d.times, d.n_frames = t["n_times"], _ptr(t["times"], C.c_double), t["n_frames"]
        d.jitter_scale, d.seed = float(t["jscale"]), int(self.seed) & 0xFFFFFFFFFFFFFFFF
        if not self.jitter:
            d.jitter = N.RTX_JITTER_OFF
        elif self.jitter_noise is not None:
            need = t["ncols"] * vc.height * vc.dof_samples * self.samples * 3
            noise = np.asarray(self.jitter_noise, np.float64).ravel()
            if noise.size < need:
                raise ValueError("jitter_noise too short: %d < %d" % (noise.size, need))
            t["noise"] = np.ascontiguousarray(noise[:need].astype(np.float32))
            d.jitter, d.noise = N.RTX_JITTER_REPLAY, _ptr(t["noise"], C.c_float)
        else:
            d.jitter = N.RTX_JITTER_PHILOX
        return d, t

    def _camera_key(self, subimage, tasks):
        """Every value camera_tables / camera_desc read, so a moved camera, new lens,
        motion or sample settings, or a new noise stream re-uploads the tables. A
        version-tracked camera (rtx.helperclasses.ViewportCamera) stands for its values
        by (identity, version); other camera objects (the reference's own, bound by
        Scene.from_reference) are compared value by value."""
        vc = self.vc
        noise = self._noise_key()
        if getattr(vc, "_untracked", True) is False:
            return (subimage, tasks, vc, vc._version, self.samples, self.jitter, self.seed, noise)
        vecs = b"".join(np.asarray(v, np.float32).tobytes() for v in (vc.position, vc.u, vc.v, vc.w))
        return (subimage, tasks, vc.width, vc.height, vc.left, vc.right, vc.top, vc.bottom, vecs, vc.d,
                vc.focal_length, vc.aperture, vc.dof_samples, tuple(vc.motion_times), self.samples, self.jitter,
                self.seed, noise)

    def _noise_key(self):
        if not (self.jitter and self.jitter_noise is not None):
            return None
        # the digest of a replayed stream is cached per array object (a new stream is a
        # new array; mutate one in place and call invalidate())
        src = self.jitter_noise
        if getattr(self, "_noise_src", None) is not src:
            a = np.ascontiguousarray(np.asarray(src, np.float64))
            self._noise_src, self._noise_digest = src, (a.size, hashlib.blake2b(a.tobytes(), digest_size=16).digest())
        return self._noise_digest

    def _set_camera(self, subimage, tasks, windows=None):
        key = self._camera_key(subimage, tasks)
        if windows is not None:  # the sequence is part of the key: render() uploads the ordinary camera again
            key += (("sequence", len(windows[0]), tuple(t for w in windows for t in w)),)
        nat = self.native()
        if self._cam_key == key:
            return self._cam_info
        d, t = self.camera_desc(subimage, tasks, windows)
        N.call("rtx_camera_set", nat.h, C.byref(d))
        self._cam_key = key
        self._cam_info = t
        self._gen = next(_GENERATION)
        return t

    # ------------------------------------------------------------------ rendering
    def render_device(self, subimage=0, tasks=1, row0=0, nrows=None, out=None, counters=None, stream=None,
                      groups=None, rgb8=False):
        """Render image rows [row0, row0 + nrows) (row 0 = top) of the strip into a float32
        CUDA tensor [nrows, strip_width, 3] (the rot90'd reference image). Asynchronous
        on ``stream`` (default: torch's current stream). ``groups=(k, n)`` instead renders
        the interleaved 8-row groups k, k + n, ... (rows ``group_rows(H, n, k)``, packed).
        A uint8 ``out`` (or rgb8=True) gets main.py's PNG bytes from the fused kernel
        (rtx_render_rgb8 / rtx_render_groups_rgb8)."""
        t = self._set_camera(subimage, tasks)
        nrows = _strip_rows(self.vc.height, row0, nrows, groups)
        shape = (nrows, t["ncols"], 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8 if rgb8 else torch.float32, device="cuda")
        rgb8 = out.dtype == torch.uint8
        _check_fb(out, tuple(out.shape) == shape, "of shape %s" % (shape,))
        cnt = _counters_ptr(counters)
        st = stream if stream is not None else torch.cuda.current_stream()
        suffix = "_rgb8" if rgb8 else ""
        if groups is not None:
            N.call("rtx_render_groups" + suffix, self._native.h, int(groups[0]), int(groups[1]),
                   C.c_void_p(out.data_ptr()), cnt, C.c_void_p(st.cuda_stream))
        else:
            N.call("rtx_render" + suffix, self._native.h, int(row0), int(nrows), C.c_void_p(out.data_ptr()), cnt,
                   C.c_void_p(st.cuda_stream))
        return out

    def render_frames(self, out, row0=0, nrows=None, stream=None, groups=None):
        """render_device(row0=row0, nrows=nrows) -- or render_device(groups=groups) -- into
        out[f, :nrows] for every frame slot f of a contiguous uint8 or float32 CUDA tensor
        out [nframes, >= nrows, W, 3], in ONE launch (rtx_render_frames /
        rtx_render_groups_frames: the frames of one scene state, e.g. a group of
        rtx.distributed.FrameExchange)."""
        t = self._set_camera(0, 1)
        nrows = _strip_rows(self.vc.height, row0, nrows, groups)
        _check_fb(out, out.dim() == 4 and out.shape[1] >= nrows and tuple(out.shape[2:]) == (t["ncols"], 3),
                  "[frames, >= %d, %d, 3]" % (nrows, t["ncols"]))
        st = stream if stream is not None else torch.cuda.current_stream()
        fn, a, b = ("rtx_render_frames", row0, nrows) if groups is None else ("rtx_render_groups_frames",) + tuple(groups)
        N.call(fn, self._native.h, int(a), int(b), C.c_void_p(out.data_ptr()), int(out.dtype == torch.uint8),
               int(out.shape[0]), int(out.stride(0) * out.element_size()), None, C.c_void_p(st.cuda_stream))
        return out

    def render_sequence(self, windows, out=None, row0=0, nrows=None, groups=None, counters=None, stream=None,
                        rgb8=False, batch=None, frames=None):
        """A frame sequence of a moving scene: frame f is what render_device renders after
        ``vc.motion_times = windows[f]``, bit for bit, without a camera upload per frame.
        ``windows`` holds F equal-length lists of motion times (rtx.frame_windows makes
        them; a flat list of numbers: one time per frame). Returns a CUDA tensor
        [F, nrows, W, 3], float32 or (rgb8=True, or a uint8 ``out``) uint8; ``out`` may have
        spare rows per slot ([F, >= nrows, W, 3]), as in render_frames. ``batch`` frames
        share one camera upload and one launch (rtx_render_sequence; default: all of them).
        The culling structures of an upload cover the time range of all its windows, so
        batches of a long sequence can render faster; the result does not depend on it.
        ``frames=(first, count)`` renders only those frames of the sequence (into ``count``
        slots). ``counters`` accumulate over all rendered frames. vc.motion_times is
        neither read nor changed; a later render() uploads the ordinary camera again."""
        windows = sequence_windows(windows)
        first, count = (0, len(windows)) if frames is None else (int(frames[0]), int(frames[1]))
        if first < 0 or count < 1 or first + count > len(windows):
            raise ValueError("frames=(first, count) must lie inside the %d windows" % len(windows))
        batch = len(windows) if batch is None else int(batch)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        H, W = self.vc.height, strip_columns(self.vc.width, 0, 1)[1]
        nrows = _strip_rows(H, row0, nrows, groups)
        if out is None:
            out = torch.empty((count, nrows, W, 3), dtype=torch.uint8 if rgb8 else torch.float32, device="cuda")
        _check_fb(out, out.dim() == 4 and out.shape[0] == count and out.shape[1] >= nrows
                  and tuple(out.shape[2:]) == (W, 3), "[%d, >= %d, %d, 3]" % (count, nrows, W))
        cnt = _counters_ptr(counters)
        st = stream if stream is not None else torch.cuda.current_stream()
        fn, a, b = ("rtx_render_sequence", row0, nrows) if groups is None else \
            ("rtx_render_groups_sequence",) + tuple(groups)
        stride = int(out.stride(0) * out.element_size())
        for k0 in range(0, count, batch):
            n = min(batch, count - k0)
            if batch >= count:  # one upload of the whole sequence: the library picks the frames
                self._set_camera(0, 1, windows)
                frame0 = first
            else:               # each batch uploads its own windows
                self._set_camera(0, 1, windows[first + k0:first + k0 + n])
                frame0 = 0
            N.call(fn, self._native.h, int(a), int(b), C.c_void_p(out.data_ptr() + k0 * stride),
                   int(out.dtype == torch.uint8), frame0, n, stride, cnt, C.c_void_p(st.cuda_stream))
        return out

    # ------------------------------------------------------------------ first-hit buffers
    def render_aovs(self, aovs=AOV_NAMES, subimage=0, tasks=1, row0=0, nrows=None, windows=None, frame=0, out=None,
                    stream=None):
        """What the first sample of each pixel sees (rtx_render_aov): a dict name -> CUDA
        tensor for the chosen ``aovs`` of image rows [row0, row0 + nrows) (row 0 = top) of
        the strip -- "depth" float32 [nrows, W] (+inf on a miss), "normal", "position" and
        "albedo" float32 [nrows, W, 3] (0), "object" and "material" int32 [nrows, W], the
        indices in ``objects`` / ``materials`` (-1). The ray is the one of DOF origin 0 and
        AA origin 0 with that sample's jitter draw, at the first motion time: for a
        one-sample camera the ray whose colour render() stores. ``windows`` (as
        render_sequence takes them) makes it the first time of window ``frame`` instead.
        ``out``: a dict of preallocated contiguous CUDA tensors for some or all of the
        names. Asynchronous on ``stream`` (default: torch's current stream)."""
        names = _buffer_names("render_aovs", "a feature buffer", AOV_NAMES, aovs)
        windows, frame = _window_frame(windows, frame)
        H, W = self.vc.height, strip_columns(self.vc.width, subimage, tasks)[1]
        row0, nrows = _row_range(H, row0, nrows)
        table = {n: ((nrows, W, 3) if n in _AOV_VEC else (nrows, W), torch.int32 if n in _AOV_INT else torch.float32)
                 for n in AOV_NAMES}
        out = _out_dict(out, names, table)
        self._set_camera(subimage, tasks, windows)
        out = _out_alloc(out, names, table)
        st = stream if stream is not None else torch.cuda.current_stream()
        ptr = [C.c_void_p(out[n].data_ptr() if n in out else 0) for n in AOV_NAMES]
        if nrows > 0:  # (the tensors of an empty block have no storage to point at)
            N.call("rtx_render_aov", self._native.h, row0, nrows, frame, *ptr, C.c_void_p(st.cuda_stream))
        return out

    def pick(self, col, row, **camera_kwargs):
        """What pixel (column ``col``, row ``row`` from the top) of the strip shows, as host
        values: a dict with "object" (the entry of ``objects``, None on a miss), "material"
        (the entry of ``materials``, or None), "depth" (float, inf), "position", "normal"
        and "albedo" (numpy float32 [3]). ``camera_kwargs``: render_aovs's subimage, tasks,
        windows, frame and stream. Renders the one image row holding the pixel."""
        for k in camera_kwargs:
            if k not in ("subimage", "tasks", "windows", "frame", "stream"):
                raise ValueError("pick takes subimage, tasks, windows, frame and stream, not %r" % k)
        col, row = int(col), int(row)
        W = strip_columns(self.vc.width, camera_kwargs.get("subimage", 0), camera_kwargs.get("tasks", 1))[1]
        if not (0 <= col < W and 0 <= row < self.vc.height):
            raise ValueError("pixel (%d, %d) outside the %d x %d strip" % (col, row, W, self.vc.height))
        b = self.render_aovs(row0=row, nrows=1, **camera_kwargs)
        if camera_kwargs.get("stream") is not None:
            camera_kwargs["stream"].synchronize()
        b = {n: t[0, col].cpu().numpy() for n, t in b.items()}
        oi, mi = int(b["object"]), int(b["material"])
        return dict(object=self.objects[oi] if oi >= 0 else None, material=self.materials[mi] if mi >= 0 else None,
                    depth=float(b["depth"]), position=b["position"], normal=b["normal"], albedo=b["albedo"])

    # ------------------------------------------------------------------ occlusion buffers
    def render_occlusion(self, buffers=OCCLUSION_NAMES, ao_samples=16, ao_radius=math.inf, ao_dirs=None, subimage=0,
                         tasks=1, row0=0, nrows=None, windows=None, frame=0, out=None, stream=None):
        """Visibility at the first hit of each pixel (rtx_render_occlusion; no reference
        counterpart): a dict name -> CUDA tensor [nrows, W] for the chosen ``buffers`` of image
        rows [row0, row0 + nrows) (row 0 = top) of the strip. The ray, the hit and the motion
        time are render_aovs' (``windows`` / ``frame`` as there); p and n are its "position" and
        "normal".

        "lights": bit i is set iff light i's shadow ray from p is free (scene.py:150-167) --
        what ``occluded`` answers for it; 0 on a miss. At most 32 lights. torch has no CUDA
        uint32 arithmetic, so the mask is handed out as **int32** holding the same bits (bit
        31 is the sign; ``.cpu().numpy().view(numpy.uint32)`` gives the unsigned words).

        "ao": float32, the share of the ambient-occlusion rays from p that are free up to
        ``ao_radius`` (> 0 or inf); 1.0 on a miss. The rays run along ``ao_dirs``, float32
        [K, 3] local directions with z along the normal (1 <= K <= 64, finite; default:
        ``cosine_directions(ao_samples)``), in the orthonormal frame rtx.h spells out. The
        hemisphere is about the stored normal, which is not flipped toward the viewer.

        ``out``: a dict of preallocated contiguous CUDA tensors for some or all of the names.
        Asynchronous on ``stream`` (default: torch's current stream)."""
        names = _buffer_names("render_occlusion", "an occlusion buffer", OCCLUSION_NAMES, buffers)
        windows, frame = _window_frame(windows, frame)
        H, W = self.vc.height, strip_columns(self.vc.width, subimage, tasks)[1]
        row0, nrows = _row_range(H, row0, nrows)
        if "lights" in names and len(self.lights) > 32:
            raise ValueError("the light mask holds 32 lights, the scene has %d" % len(self.lights))
        dirs, radius = None, math.inf
        if "ao" in names:
            if ao_dirs is None:
                if isinstance(ao_samples, bool) or not isinstance(ao_samples, (int, np.integer)) \
                        or not 1 <= ao_samples <= N.RTX_AO_MAX_DIRS:
                    raise ValueError("ao_samples must be an integer in [1, %d], got %r" % (N.RTX_AO_MAX_DIRS, ao_samples))
                dirs = cosine_directions(int(ao_samples))
            else:
                try:
                    with np.errstate(over="ignore"):
                        dirs = np.ascontiguousarray(np.asarray(ao_dirs, np.float64).astype(np.float32))
                except (TypeError, ValueError):
                    raise ValueError("ao_dirs must be an array of shape [K, 3]") from None
                if dirs.ndim != 2 or dirs.shape[1] != 3 or not 1 <= dirs.shape[0] <= N.RTX_AO_MAX_DIRS:
                    raise ValueError("ao_dirs must have shape [K, 3] with 1 <= K <= %d, not %s"
                                     % (N.RTX_AO_MAX_DIRS, dirs.shape))
                if not np.isfinite(dirs).all():
                    raise ValueError("ao_dirs must be finite (as fp32)")
            try:
                radius = float(ao_radius)
            except (TypeError, ValueError):
                raise ValueError("ao_radius must be a number") from None
            if not radius > 0.0:  # (NaN too)
                raise ValueError("ao_radius must be > 0 or inf, got %r" % (ao_radius,))
        table = dict(lights=((nrows, W), torch.int32), ao=((nrows, W), torch.float32))
        out = _out_dict(out, names, table)
        self._set_camera(subimage, tasks, windows)
        out = _out_alloc(out, names, table)
        st = stream if stream is not None else torch.cuda.current_stream()
        if nrows > 0:  # (the tensors of an empty block have no storage to point at)
            vp = C.c_void_p
            N.call("rtx_render_occlusion", self._native.h, row0, nrows, frame,
                   vp(out["lights"].data_ptr() if "lights" in out else 0), vp(out["ao"].data_ptr() if "ao" in out else 0),
                   _ptr(dirs, C.c_float) if dirs is not None else None, 0 if dirs is None else int(dirs.shape[0]),
                   radius, vp(st.cuda_stream))
        return out

    # ------------------------------------------------------------------ resolved buffers
    def _matte_indices(self, matte):
        """``matte`` (object indices, or entries of ``objects`` matched by identity) as a
        contiguous int32 array of indices into ``objects``."""
        if matte is None:
            raise ValueError('the "matte" buffer needs matte=: a non-empty sequence of objects or object indices')
        try:
            items = list(matte)
        except TypeError:
            raise ValueError("matte must be a sequence of objects or object indices") from None
        if not items:
            raise ValueError("matte must name at least one object")
        n = len(self.objects)
        idx = []
        for m in items:
            if isinstance(m, (int, np.integer)) and not isinstance(m, bool):
                i = int(m)
            else:
                i = next((k for k, ob in enumerate(self.objects) if ob is m), None)
                if i is None:
                    raise ValueError("matte entry %r is neither an object index nor one of scene.objects" % (m,))
            if not 0 <= i < n or i >= N.RTX_MATTE_MAX_OBJECTS:
                raise ValueError("matte object %d outside the scene's %d objects (a matte holds indices below %d)"
                                 % (i, n, N.RTX_MATTE_MAX_OBJECTS))
            idx.append(i)
        return np.ascontiguousarray(idx, np.int32)

    def render_resolved(self, buffers=("alpha", "depth", "normal", "albedo"), matte=None, subimage=0, tasks=1, row0=0,
                        nrows=None, windows=None, frame=0, out=None, stream=None):
        """What each pixel covers over ALL its samples (rtx_render_resolved; no reference
        counterpart): a dict name -> float32 CUDA tensor for the chosen ``buffers`` of image
        rows [row0, row0 + nrows) (row 0 = top) of the strip. The samples are the render's:
        every DOF origin, AA origin (with the render's jitter draw) and motion time, so the
        buffers line up with the colour render_device stores, where render_aovs describes
        the first sample only. With S samples per pixel, H of them hits:

        "alpha" [nrows, W]: H / S, the coverage. "matte" [nrows, W]: the share of the samples
        whose first hit lies on an object of ``matte`` -- a non-empty sequence of indices into
        ``objects`` or of its entries (matched by identity; duplicates allowed, indices below
        256); it may be asked for only with ``matte``. "depth" [nrows, W]: the mean of
        render_aovs' depth over the hits (inf when H == 0). "normal" and "albedo"
        [nrows, W, 3]: the sums of render_aovs' values over the hits divided by S -- a miss
        adds nothing, so they are premultiplied by the coverage like the colour. All sums are
        fp32 in sample order (DOF, AA, time; time fastest). For a one-sample camera the
        buffers equal render_aovs' as values.

        Flat scenes only: a scene with hierarchies or textures gets RtxError
        (RTX_ERR_UNSUPPORTED) from the entry point.

        ``windows`` / ``frame`` as in render_aovs: the motion times of window ``frame``.
        ``out``: a dict of preallocated contiguous CUDA tensors for some or all of the names.
        Asynchronous on ``stream`` (default: torch's current stream); never synchronises."""
        names = _buffer_names("render_resolved", "a resolved buffer", RESOLVED_NAMES, buffers)
        windows, frame = _window_frame(windows, frame)
        H, W = self.vc.height, strip_columns(self.vc.width, subimage, tasks)[1]
        row0, nrows = _row_range(H, row0, nrows)
        # (a matte without its buffer is checked and otherwise ignored, as the entry point does)
        idx = self._matte_indices(matte) if "matte" in names or matte is not None else None
        if "matte" not in names:
            idx = None
        table = {n: ((nrows, W, 3) if n in _RESOLVED_VEC else (nrows, W), torch.float32) for n in RESOLVED_NAMES}
        out = _out_dict(out, names, table)
        self._set_camera(subimage, tasks, windows)
        out = _out_alloc(out, names, table)
        st = stream if stream is not None else torch.cuda.current_stream()
        ptr = [C.c_void_p(out[n].data_ptr() if n in out else 0) for n in RESOLVED_NAMES]
        if nrows > 0:  # (the tensors of an empty block have no storage to point at)
            N.call("rtx_render_resolved", self._native.h, row0, nrows, frame, *ptr,
                   _ptr(idx, C.c_int32) if idx is not None else None, 0 if idx is None else int(idx.size),
                   C.c_void_p(st.cuda_stream))
        return out

    # ------------------------------------------------------------------ ranked id-coverage buffers
    def render_ids(self, ranks=4, key="object", buffers=ID_NAMES, subimage=0, tasks=1, row0=0, nrows=None,
                   windows=None, frame=0, out=None, stream=None):
        """Which objects or materials cover each pixel, over ALL its samples (rtx_render_ids; no
        reference counterpart): a dict name -> int32 CUDA tensor for the chosen ``buffers`` of
        image rows [row0, row0 + nrows) (row 0 = top) of the strip. One pass gives the matte of
        every object of the frame (`id_matte`), where render_resolved's "matte" takes one pass
        per object set. The samples are render_resolved's. Each sample that hits has a key:
        ``key="object"`` the index in ``objects`` (render_aovs' "object"), ``key="material"``
        the index in ``materials`` (its "material").

        A pixel keeps its first 8 distinct keys in sample order with exact sample counts, and
        ranks them by count descending, equal counts by key ascending. "ids" [nrows, W, ranks]:
        the key of each rank, -1 for an empty rank. "counts" [nrows, W, ranks]: its samples, 0
        for an empty rank. "other" [nrows, W]: the hits in no written rank (keys past the
        eighth, and ranks >= ``ranks``). So counts.sum(-1) + other is the pixel's hit count, and
        where other == 0 the ranks are the pixel's complete id histogram. 1 <= ranks <= 8.

        Flat scenes only: a scene with hierarchies or textures gets RtxError
        (RTX_ERR_UNSUPPORTED) from the entry point.

        ``windows`` / ``frame`` as in render_aovs: the motion times of window ``frame``.
        ``out``: a dict of preallocated contiguous CUDA tensors for some or all of the names.
        Asynchronous on ``stream`` (default: torch's current stream); never synchronises."""
        names = _buffer_names("render_ids", "an id buffer", ID_NAMES, buffers)
        if isinstance(ranks, bool) or not isinstance(ranks, (int, np.integer)) or not 1 <= ranks <= N.RTX_ID_SLOTS:
            raise ValueError("ranks must be an integer in [1, %d], got %r" % (N.RTX_ID_SLOTS, ranks))
        if not isinstance(key, str) or key not in _ID_KEYS:
            raise ValueError("unknown id key %r (known: %s)" % (key, ", ".join(_ID_KEYS)))
        ranks = int(ranks)
        windows, frame = _window_frame(windows, frame)
        H, W = self.vc.height, strip_columns(self.vc.width, subimage, tasks)[1]
        row0, nrows = _row_range(H, row0, nrows)
        table = dict(ids=((nrows, W, ranks), torch.int32), counts=((nrows, W, ranks), torch.int32),
                     other=((nrows, W), torch.int32))
        out = _out_dict(out, names, table)
        self._set_camera(subimage, tasks, windows)
        out = _out_alloc(out, names, table)
        st = stream if stream is not None else torch.cuda.current_stream()
        ptr = [C.c_void_p(out[n].data_ptr() if n in out else 0) for n in ID_NAMES]
        if nrows > 0:  # (the tensors of an empty block have no storage to point at)
            N.call("rtx_render_ids", self._native.h, row0, nrows, frame, _ID_KEYS[key], ranks, *ptr,
                   C.c_void_p(st.cuda_stream))
        return out

    # ------------------------------------------------------------------ light groups
    def render_light_groups(self, groups=None, ambient="own", subimage=0, tasks=1, row0=0, nrows=None, windows=None,
                            frame=0, out=None, stream=None):
        """The colour render_device stores, separated by light set, in one pass
        (rtx_render_light_groups; no reference counterpart): a float32 CUDA tensor
        [G, nrows, W, 3] for image rows [row0, row0 + nrows) (row 0 = top) of the strip.
        Plane g is, bit for bit, render_device's image of this scene with only the lights of
        ``groups[g]`` (in their order) and, unless g is the ambient's group, a zero ambient.

        ``groups``: a sequence of sequences of indices into ``lights`` (None: one group per
        light); a light in no group lights nothing. ``ambient``: "own" (a group appended last),
        a group index, or None (dropped). At most 8 groups, the ambient's own included, and at
        most 32 lights. The ray chains and shadow rays are traced once, whatever the grouping.
        The planes are clamped per chain level like the image, so they sum to it only where no
        clamp engages (and then up to fp32 rounding).

        Flat scenes only: a scene with hierarchies or textures gets RtxError
        (RTX_ERR_UNSUPPORTED) from the entry point.

        ``windows`` / ``frame`` as in render_aovs: the motion times of window ``frame``.
        ``out``: a preallocated contiguous float32 CUDA tensor [G, nrows, W, 3].
        Asynchronous on ``stream`` (default: torch's current stream); never synchronises."""
        table, n_groups, ambient_group = light_group_table(len(self.lights), groups, ambient)
        if len(self.lights) > 32:
            raise ValueError("a light-group pass holds 32 lights, the scene has %d" % len(self.lights))
        windows, frame = _window_frame(windows, frame)
        H, W = self.vc.height, strip_columns(self.vc.width, subimage, tasks)[1]
        row0, nrows = _row_range(H, row0, nrows)
        shape = (n_groups, nrows, W, 3)
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape
                                or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous()):
            raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
        self._set_camera(subimage, tasks, windows)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device="cuda")
        st = stream if stream is not None else torch.cuda.current_stream()
        if nrows > 0:  # (the tensor of an empty block has no storage to point at)
            arg = table if table.size else np.full(1, -1, np.int32)  # (never a null pointer: no lights)
            N.call("rtx_render_light_groups", self._native.h, row0, nrows, frame, _ptr(arg, C.c_int32), n_groups,
                   ambient_group, C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream))
        return out

    def id_matte(self, ids, counts, members, samples=None):
        """`id_matte` of render_ids' object-key buffers for ``members`` as render_resolved takes
        its ``matte``: object indices or entries of ``objects`` (matched by identity).
        ``samples``: the samples per pixel of the pass (default: samples_per_pixel, the
        camera's own motion times)."""
        idx = self._matte_indices(members)
        return id_matte(ids, counts, [int(i) for i in idx], self.samples_per_pixel if samples is None else samples)

    def render(self, subimage: int = 0, tasks: int = 1) -> np.ndarray:
        """scene.py:35-79 — returns float64 (strip_width, height, 3), [column, row-from-bottom]."""
        fb = self.render_device(subimage, tasks)
        img = fb.cpu().numpy()
        return np.ascontiguousarray(np.transpose(img[::-1], (1, 0, 2))).astype(np.float64)

    def render_rgb8(self, subimage=0, tasks=1):
        """main.py:31-33 on the device: (rot90(image) * 255).astype(uint8), (H, W, 3)."""
        return self.render_device(subimage, tasks, rgb8=True).cpu().numpy()

    # ------------------------------------------------------------------ Geometry ABI (batched)
    def intersect(self, origins, directions, time=0.0):
        """Closest hit of rays [n, 3] (Geometry.intersect over all objects + min by time,
        scene.py:86-94). Returns dict of numpy arrays: t (inf on miss), obj (-1), mat (-1),
        normal [n, 3], position [n, 3]."""
        nat = self.native()
        o = torch.as_tensor(np.ascontiguousarray(np.asarray(origins, np.float32).reshape(-1, 3).T)).cuda()
        d = torch.as_tensor(np.ascontiguousarray(np.asarray(directions, np.float32).reshape(-1, 3).T)).cuda()
        n = o.shape[1]
        t = torch.empty(n, dtype=torch.float64, device="cuda")
        ob = torch.empty(n, dtype=torch.int32, device="cuda")
        m = torch.empty(n, dtype=torch.int32, device="cuda")
        nn = torch.empty((3, n), dtype=torch.float32, device="cuda")
        pp = torch.empty((3, n), dtype=torch.float32, device="cuda")
        vp = C.c_void_p
        N.call("rtx_intersect", nat.h, n, vp(o.data_ptr()), vp(d.data_ptr()), float(time), vp(t.data_ptr()),
               vp(ob.data_ptr()), vp(m.data_ptr()), vp(nn.data_ptr()), vp(pp.data_ptr()),
               vp(torch.cuda.current_stream().cuda_stream))
        return dict(t=t.cpu().numpy(), obj=ob.cpu().numpy(), mat=m.cpu().numpy(),
                    normal=nn.cpu().numpy().T.copy(), position=pp.cpu().numpy().T.copy())

    def occluded(self, origins, directions, t_max, time=0.0):
        """Shadow any-hit (Geometry.shadow_intersect over all objects, scene.py:160-164)."""
        nat = self.native()
        o = torch.as_tensor(np.ascontiguousarray(np.asarray(origins, np.float32).reshape(-1, 3).T)).cuda()
        d = torch.as_tensor(np.ascontiguousarray(np.asarray(directions, np.float32).reshape(-1, 3).T)).cuda()
        n = o.shape[1]
        tm = torch.as_tensor(np.array(np.broadcast_to(np.asarray(t_max, np.float64), (n,)))).cuda()
        occ = torch.empty(n, dtype=torch.uint8, device="cuda")
        vp = C.c_void_p
        N.call("rtx_occluded", nat.h, n, vp(o.data_ptr()), vp(d.data_ptr()), vp(tm.data_ptr()), float(time),
               vp(occ.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
        return occ.cpu().numpy().astype(bool)

    # ------------------------------------------------------------------ shading caller-built rays
    def camera_rays(self, subimage=0, tasks=1, device=False):
        """The reference camera's sample rays of the strip (scene.py:54-65), in fp32 from
        camera_tables: (origins [n, 3], directions [n, 3], group) as numpy float32 arrays,
        ordered image row (row 0 = top), column, DOF origin, AA origin, with
        group = dof_samples * samples rays per pixel; replayed jitter (jitter_noise) moves
        the origins as scene.py:63-65 does. ``device=True``: the rays as contiguous float32
        CUDA tensors [3, n] instead, what cast_rays_device takes -- then
        ``cast_rays_device(o, d, vc.motion_times, group).view(H, W, 3)`` is
        ``render_device(subimage, tasks)`` bit for bit. ValueError for Philox jitter, whose
        draws exist only on the device."""
        if self.jitter and self.jitter_noise is None:
            raise ValueError("camera_rays needs replayed jitter (jitter_noise): Philox draws exist only on the device")
        t = self.camera_tables(subimage, tasks)
        vc = self.vc
        f32 = np.float32
        H, W, nd, na = vc.height, t["ncols"], vc.dof_samples, self.samples
        u, v, w = (np.asarray(x, f32) for x in (vc.u, vc.v, vc.w))
        xs, ys = t["xs"], t["ys"][::-1]  # image row r is the reference's row H - 1 - r
        bdir = F.normalize((xs[None, :, None] * u + ys[:, None, None] * v) - w * f32(vc.d))  # scene.py:54
        focal = np.asarray(vc.position, f32) + bdir * f32(vc.focal_length)                    # scene.py:55
        dof = t["dof"].astype(f32).reshape(nd, 3)
        d = F.normalize(focal[:, :, None, :] - dof[None, None])                               # scene.py:58
        d = np.broadcast_to(d[:, :, :, None, :], (H, W, nd, na, 3))
        o = np.broadcast_to(t["aa"].astype(f32).reshape(nd, na, 3), (H, W, nd, na, 3))        # scene.py:60-61
        if self.jitter:                                                                       # scene.py:63-65
            need = W * H * nd * na * 3
            noise = np.asarray(self.jitter_noise, np.float64).ravel()
            if noise.size < need:
                raise ValueError("jitter_noise too short: %d < %d" % (noise.size, need))
            # the reference draws per column, then per row from the bottom
            nz = noise[:need].astype(f32).reshape(W, H, nd, na, 3).transpose(1, 0, 2, 3, 4)[::-1]
            o = o + F.normalize(nz) * f32(t["jscale"])
        o = np.ascontiguousarray(o, f32).reshape(-1, 3)
        d = np.ascontiguousarray(d, f32).reshape(-1, 3)
        if device:
            return (torch.as_tensor(np.ascontiguousarray(o.T)).cuda(), torch.as_tensor(np.ascontiguousarray(d.T)).cuda(),
                    nd * na)
        return o, d, nd * na

    @staticmethod
    def _cast_args(n, times, group):
        """cast_rays' motion times (a number or a sequence of 1 .. RTX_CAST_MAX_TIMES finite
        numbers) as a float64 array, and ``group`` checked against the n rays."""
        try:
            ts = np.atleast_1d(np.asarray(times, np.float64))
        except (TypeError, ValueError):
            raise ValueError("times must be a number or a sequence of numbers") from None
        if ts.ndim != 1 or not 1 <= ts.size <= N.RTX_CAST_MAX_TIMES:
            raise ValueError("cast_rays takes 1 to %d motion times, got %s" % (N.RTX_CAST_MAX_TIMES, ts.shape))
        with np.errstate(over="ignore"):
            finite = np.isfinite(ts).all() and np.isfinite(ts.astype(np.float32)).all()
        if not finite:
            raise ValueError("motion times must be finite (as fp32)")
        if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or group < 1:
            raise ValueError("group must be an integer >= 1, got %r" % (group,))
        if n % group:
            raise ValueError("group %d does not divide the %d rays" % (group, n))
        if int(group) * ts.size > 0x7FFFFFFF:
            raise ValueError("group * len(times) must stay below 2^31")
        return np.ascontiguousarray(ts), int(group)

    def cast_rays_device(self, o, d, times=0.0, group=1, out=None, counters=None, stream=None):
        """Scene.cast_ray (scene.py:81-116) for caller-built rays, batched (rtx_cast_rays):
        ``o`` and ``d`` are contiguous float32 CUDA tensors [3, n] (origins, directions; the
        directions are used as given, not normalised). Every ray is cast at every motion time
        of ``times``; each run of ``group`` rays gives one colour, the fp32 mean of its
        group * len(times) samples added in order (ray, then time) -- a pixel's loop nest.
        Returns a float32 CUDA tensor [n / group, 3] (``out`` when given), which
        fb_to_rgb8 takes. ``counters`` accumulate like render_device's. Uses nothing of the
        camera and needs none. Asynchronous on ``stream`` (default: torch's current
        stream); never synchronises."""
        for name, a in (("o", o), ("d", d)):
            if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.dim() != 2 or a.shape[0] != 3 \
                    or not a.is_contiguous():
                raise ValueError("%s must be a contiguous float32 tensor of shape [3, n]" % name)
        if o.shape != d.shape:
            raise ValueError("o and d hold different numbers of rays: %d and %d" % (o.shape[1], d.shape[1]))
        n = int(o.shape[1])
        ts, group = self._cast_args(n, times, group)
        shape = (n // group, 3)
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape
                                or out.dtype != torch.float32 or not out.is_contiguous()):
            raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
        if counters is not None and (not isinstance(counters, torch.Tensor) or counters.numel() < N.RTX_COUNTERS
                                     or counters.dtype != torch.int64):
            raise ValueError("counters must be an int64 CUDA tensor with >= %d entries" % N.RTX_COUNTERS)
        for name, a in (("o", o), ("d", d), ("out", out), ("counters", counters)):
            if a is not None and (not a.is_cuda or a.device != o.device):
                raise ValueError("%s must be a CUDA tensor on the rays' device" % name)
        nat = self.native()
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=o.device)
        st = stream if stream is not None else torch.cuda.current_stream()
        vp = C.c_void_p
        N.call("rtx_cast_rays", nat.h, n, vp(o.data_ptr()), vp(d.data_ptr()), _ptr(ts, C.c_double), int(ts.size), group,
               vp(out.data_ptr()), vp(counters.data_ptr() if counters is not None else 0), vp(st.cuda_stream))
        return out

    def cast_rays(self, origins, directions, times=0.0, group=1):
        """cast_rays_device for numpy rays [n, 3] (like intersect): returns the colours as a
        numpy float32 array [n / group, 3]."""
        o = np.asarray(origins, np.float32)
        d = np.asarray(directions, np.float32)
        for name, a in (("origins", o), ("directions", d)):
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError("%s must have shape [n, 3], not %s" % (name, a.shape))
        if o.shape != d.shape:
            raise ValueError("origins and directions hold different numbers of rays: %d and %d"
                             % (o.shape[0], d.shape[0]))
        self._cast_args(o.shape[0], times, group)
        od = torch.as_tensor(np.ascontiguousarray(o.T)).cuda()
        dd = torch.as_tensor(np.ascontiguousarray(d.T)).cuda()
        return self.cast_rays_device(od, dd, times, group).cpu().numpy()

    @property
    def samples_per_pixel(self):
        """AA origins x DOF origins x the camera's motion times: S of render_resolved and render_ids."""
        return self.samples * self.vc.dof_samples * len(self.vc.motion_times)
