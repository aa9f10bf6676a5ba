"""CLI mirror of provided/main.py:14-35.

    python -m rtx.main --infile S.json --outfile out.png [--subimage k --tasks N]

Full render: rot90 + truncating uint8 conversion + PNG (main.py:29-34; the viewer call
`im.show()` at :35 is not reproduced). Strip render: numpy.save of the (strip_w, H, 3)
float64 strip (main.py:26-28), for rtx.glue. Extensions: --resolution W H and --spp AA [DOF]
edit the scene like the bench configs; --distributed renders row blocks on every rank
of a torch.distributed job and gathers the frame to rank 0 (render.nu's role).

    python -m rtx.main --infile S.json --frames N [--time-range T0 T1]
                       [--shutter S --shutter-samples M] --outfile out.png

A frame sequence of a moving scene (no reference counterpart): N frames opening at equal
steps over [T0, T1) -- default 0 .. the scene's last motion time -- each blurred over S
time units with M samples (default: one time per frame), rendered by
Scene.render_sequence in batches and written as out_0000.png, out_0001.png, ... (or through
a %d pattern in the name, e.g. frame%03d.png).

    python -m rtx.main --infile S.json --outfile out.png --aovs out.npz [--aov-names depth normal ...]

Besides the image, the first-hit feature buffers of Scene.render_aovs (no reference
counterpart; default: all six) as (H, W) or (H, W, 3) arrays of one .npz file.

    python -m rtx.main --infile S.json --outfile pano.png --panorama W H

An equirectangular W x H panorama about the scene's camera position (no reference
counterpart: rtx.panorama_rays shaded by Scene.cast_rays_device at the camera's motion times),
in place of the camera's image.

    python -m rtx.main --infile S.json --outfile out.png --occlusion occ.npz [--ao-samples K] [--ao-radius R]

Besides the image, the occlusion buffers of Scene.render_occlusion (no reference counterpart)
as (H, W) arrays of one .npz file: `lights` (uint32, bit i: light i reaches the pixel's first
hit) and `ao` (float32, the share of K ambient-occlusion rays of length R that are free;
default 16 rays, unbounded).

    python -m rtx.main --infile S.json --outfile out.png --resolved res.npz [--resolved-names alpha depth ...]
                       [--matte-objects I ...] [--rgba out_rgba.png]

Besides the image, the all-sample buffers of Scene.render_resolved (no reference counterpart)
as (H, W) or (H, W, 3) float32 arrays of one .npz file: `alpha` (the pixel's coverage), `depth`
(the mean over the samples that hit), `normal` and `albedo` (means over all samples, so
premultiplied by the coverage like the colour), and -- with --matte-objects, the indices of the
scene's objects that make up the matte -- `matte` (the share of the samples that see one of
them). Default: alpha depth normal albedo, plus matte when --matte-objects is given.

--rgba FILE.png writes the frame as an RGBA PNG for compositing: its RGB bytes are exactly
--outfile's and A is the truncated (alpha * 255). The colour is ASSOCIATED (premultiplied)
alpha over the reference's black background: a sample that misses adds black to the pixel, so
the frame goes over a background B as RGB + (1 - A) * B, with no multiplication of RGB by A.

    python -m rtx.main --infile S.json --outfile out.png --ids ids.npz [--id-ranks K] [--id-key object|material]

Besides the image, the ranked id-coverage buffers of Scene.render_ids (no reference counterpart)
as one .npz file: `ids` and `counts` (int32 (H, W, K): per pixel the K objects -- or materials --
that cover the most samples and their sample counts, -1 / 0 for an empty rank), `other` (int32
(H, W): the hits in no written rank), `samples` (the samples per pixel, a scalar) and `names`
(the objects' or the materials' names in index order). Default: 4 ranks, the object key. The
matte of any set of objects is then sum(counts where ids is in the set) / samples.
"""
import argparse
import json
import os

import numpy

from ._native import RTX_AO_MAX_DIRS, RTX_ID_SLOTS
from .scene import AOV_NAMES, ID_NAMES, RESOLVED_NAMES

RESOLVED_DEFAULT = ("alpha", "depth", "normal", "albedo")
ID_KEYS = ("object", "material")


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--infile", type=str, help="Name of json file that will define the scene")
    p.add_argument("--outfile", type=str, default="out.png", help="Name of png that will contain the render")
    p.add_argument("--subimage", type=int, required=False)
    p.add_argument("--tasks", type=int, required=False)
    p.add_argument("--resolution", type=int, nargs=2, default=None)
    p.add_argument("--spp", type=int, nargs="+", default=None, help="AA samples [DOF samples]")
    p.add_argument("--distributed", action="store_true")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--frames", type=int, default=None, help="render a sequence of this many frames")
    p.add_argument("--time-range", type=float, nargs=2, default=None, metavar=("T0", "T1"),
                   help="motion times the sequence spans (default: 0 .. the scene's last motion time)")
    p.add_argument("--shutter", type=float, default=0.0, help="time each frame is blurred over")
    p.add_argument("--shutter-samples", type=int, default=1, help="motion times per frame")
    p.add_argument("--aovs", type=str, default=None, metavar="FILE.npz",
                   help="also write the first-hit feature buffers (Scene.render_aovs) to this .npz file")
    p.add_argument("--aov-names", type=str, nargs="+", default=None, metavar="NAME",
                   help="the buffers to write (default: depth normal position albedo object material)")
    p.add_argument("--panorama", type=int, nargs=2, default=None, metavar=("W", "H"),
                   help="write an equirectangular W x H panorama about the camera position instead of its image")
    p.add_argument("--occlusion", type=str, default=None, metavar="FILE.npz",
                   help="also write the occlusion buffers (Scene.render_occlusion: lights, ao) to this .npz file")
    p.add_argument("--ao-samples", type=int, default=None, metavar="K",
                   help="ambient-occlusion rays per pixel, 1 .. 64 (default 16)")
    p.add_argument("--ao-radius", type=float, default=None, metavar="R",
                   help="length of the ambient-occlusion rays, > 0 (default: unbounded)")
    p.add_argument("--resolved", type=str, default=None, metavar="FILE.npz",
                   help="also write the all-sample buffers (Scene.render_resolved) to this .npz file")
    p.add_argument("--resolved-names", type=str, nargs="+", default=None, metavar="NAME",
                   help="the buffers to write (default: alpha depth normal albedo; matte with --matte-objects)")
    p.add_argument("--matte-objects", type=int, nargs="+", default=None, metavar="I",
                   help="indices of the scene's objects whose share of each pixel the `matte` buffer holds")
    p.add_argument("--rgba", type=str, default=None, metavar="FILE.png",
                   help="also write the frame as an RGBA PNG: --outfile's RGB bytes with the coverage as A "
                        "(associated alpha over the reference's black background)")
    p.add_argument("--ids", type=str, default=None, metavar="FILE.npz",
                   help="also write the ranked id-coverage buffers (Scene.render_ids) to this .npz file")
    p.add_argument("--id-ranks", type=int, default=None, metavar="K",
                   help="ranks per pixel, 1 .. %d (default 4)" % RTX_ID_SLOTS)
    p.add_argument("--id-key", type=str, default=None, choices=ID_KEYS,
                   help="what a sample is counted under (default object)")
    args = p.parse_args(argv)
    if args.ids is not None:
        if args.distributed:
            p.error("--ids renders on one GPU: it cannot be combined with --distributed")
        if args.frames is not None or args.panorama is not None:
            p.error("--ids writes the buffers of the camera's one frame: it cannot be combined with --frames or "
                    "--panorama")
        if args.id_ranks is not None and not 1 <= args.id_ranks <= RTX_ID_SLOTS:
            p.error("--id-ranks takes 1 .. %d" % RTX_ID_SLOTS)
    elif args.id_ranks is not None or args.id_key is not None:
        p.error("--id-ranks and --id-key need --ids")
    if args.resolved is not None or args.rgba is not None:
        if args.distributed:
            p.error("--resolved and --rgba render on one GPU: they cannot be combined with --distributed")
        if args.frames is not None or args.panorama is not None:
            p.error("--resolved and --rgba write the buffers of the camera's one frame: they cannot be combined "
                    "with --frames or --panorama")
    if args.rgba is not None and (args.subimage is not None or args.tasks is not None):
        p.error("--rgba writes a whole image: it cannot be combined with --subimage / --tasks")
    if args.resolved is not None:
        names = args.resolved_names
        if names is not None and (len(set(names)) != len(names) or not set(names) <= set(RESOLVED_NAMES)):
            p.error("--resolved-names takes distinct names out of: " + " ".join(RESOLVED_NAMES))
        if names is not None and ("matte" in names) != (args.matte_objects is not None):
            p.error("the matte buffer and --matte-objects need each other")
        if args.matte_objects is not None and min(args.matte_objects) < 0:
            p.error("--matte-objects takes object indices >= 0")
    elif args.resolved_names is not None or args.matte_objects is not None:
        p.error("--resolved-names and --matte-objects need --resolved")
    if args.occlusion is not None:
        if args.distributed:
            p.error("--occlusion renders on one GPU: it cannot be combined with --distributed")
        if args.frames is not None or args.panorama is not None:
            p.error("--occlusion writes the buffers of the camera's one frame: it cannot be combined with "
                    "--frames or --panorama")
        if args.ao_samples is not None and not 1 <= args.ao_samples <= RTX_AO_MAX_DIRS:
            p.error("--ao-samples takes 1 .. %d" % RTX_AO_MAX_DIRS)
        if args.ao_radius is not None and not args.ao_radius > 0.0:
            p.error("--ao-radius must be > 0")
    elif args.ao_samples is not None or args.ao_radius is not None:
        p.error("--ao-samples and --ao-radius need --occlusion")
    if args.panorama is not None:
        if args.distributed or args.frames is not None or args.aovs is not None or args.subimage is not None \
                or args.tasks is not None:
            p.error("--panorama writes one whole image on one GPU: it cannot be combined with --distributed, "
                    "--frames, --aovs or --subimage / --tasks")
        if min(args.panorama) < 1:
            p.error("--panorama takes a width and a height >= 1")
    if args.aovs is not None:
        if args.distributed:
            p.error("--aovs renders on one GPU: it cannot be combined with --distributed")
        if args.frames is not None:
            p.error("--aovs writes the buffers of one frame: it cannot be combined with --frames")
        if args.aov_names is not None and (len(set(args.aov_names)) != len(args.aov_names)
                                           or not set(args.aov_names) <= set(AOV_NAMES)):
            p.error("--aov-names takes distinct names out of: " + " ".join(AOV_NAMES))
    elif args.aov_names is not None:
        p.error("--aov-names needs --aovs")
    if args.frames is not None:
        if args.distributed or args.subimage is not None or args.tasks is not None:
            p.error("--frames renders whole frames on one GPU: it cannot be combined with --distributed or "
                    "--subimage / --tasks")
        if args.frames < 1 or args.shutter_samples < 1:
            p.error("--frames and --shutter-samples must be >= 1")
        try:
            frame_names(args.outfile, 1)
        except (TypeError, ValueError):
            p.error("--outfile may hold one integer pattern such as %%04d, not %r" % args.outfile)
    elif args.time_range is not None or args.shutter != 0.0 or args.shutter_samples != 1:
        p.error("--time-range, --shutter and --shutter-samples need --frames")
    return args


def frame_names(outfile, frames):
    """The sequence's file names: ``outfile`` % f when it holds a pattern such as %04d, else
    the frame number (at least four digits) goes before the extension: out.png -> out_0000.png."""
    if "%" in outfile:
        return [outfile % f for f in range(frames)]
    root, ext = os.path.splitext(outfile)
    return ["%s_%04d%s" % (root, f, ext) for f in range(frames)]


# Frames per camera upload and launch of a CLI sequence: the frames of a batch wait on the
# device as uint8 (this many bytes at most), and a batch's culling structures cover only its
# own time range.
SEQUENCE_BATCH_BYTES = 256 << 20
SEQUENCE_BATCH_FRAMES = 64


def render_frames_to_files(sc, args):
    from PIL import Image
    from .scene import frame_windows
    t0, t1 = args.time_range if args.time_range is not None else (0.0, float(sc.vc.motion_times[-1]))
    windows = frame_windows(t0, t1, args.frames, args.shutter, args.shutter_samples)
    names = frame_names(args.outfile, args.frames)
    batch = max(1, min(SEQUENCE_BATCH_FRAMES, SEQUENCE_BATCH_BYTES // (sc.vc.width * sc.vc.height * 3)))
    for f0 in range(0, args.frames, batch):
        rgb = sc.render_sequence(windows[f0:f0 + batch], rgb8=True).cpu().numpy()
        # the scene-specialized kernels compile on a host thread while the generic ones render
        # (option jit_async): wait for them, so that the later batches run them and a short
        # sequence does not end the process with a compile still running
        sc.jit_wait()
        for k, img in enumerate(rgb):
            Image.fromarray(img).save(names[f0 + k])
    return names


def write_aovs(sc, args):
    """The chosen feature buffers of the frame (or strip) as one .npz file: name -> (H, W) or
    (H, W, 3) array, row 0 at the top."""
    names = tuple(args.aov_names) if args.aov_names is not None else AOV_NAMES
    kw = {}
    if args.subimage is not None and args.tasks is not None:
        kw = dict(subimage=args.subimage, tasks=args.tasks)
    buffers = sc.render_aovs(names, **kw)
    with open(args.aovs, "wb") as f:  # (numpy.savez would append ".npz" to a bare name)
        numpy.savez(f, **{n: buffers[n].cpu().numpy() for n in names})
    return args.aovs


def write_occlusion(sc, args):
    """The occlusion buffers of the frame (or strip) as one .npz file: `lights` uint32 and `ao`
    float32, (H, W) arrays, row 0 at the top."""
    kw = {}
    if args.subimage is not None and args.tasks is not None:
        kw = dict(subimage=args.subimage, tasks=args.tasks)
    if args.ao_samples is not None:
        kw["ao_samples"] = args.ao_samples
    if args.ao_radius is not None:
        kw["ao_radius"] = args.ao_radius
    b = sc.render_occlusion(("lights", "ao"), **kw)
    with open(args.occlusion, "wb") as f:  # (numpy.savez would append ".npz" to a bare name)
        # (the device tensor is int32 holding the mask's bits: torch has no CUDA uint32 arithmetic)
        numpy.savez(f, lights=b["lights"].cpu().numpy().view(numpy.uint32), ao=b["ao"].cpu().numpy())
    return args.occlusion


def resolved_names(args):
    """The buffers --resolved writes: the chosen ones, else the default set (with the matte when
    --matte-objects names one)."""
    if args.resolved_names is not None:
        return tuple(args.resolved_names)
    return RESOLVED_DEFAULT + (("matte",) if args.matte_objects is not None else ())


def write_resolved(sc, args):
    """The chosen all-sample buffers of the frame (or strip) as one .npz file: name -> float32
    (H, W) or (H, W, 3) array, row 0 at the top."""
    names = resolved_names(args)
    kw = {}
    if args.subimage is not None and args.tasks is not None:
        kw = dict(subimage=args.subimage, tasks=args.tasks)
    buffers = sc.render_resolved(names, matte=args.matte_objects, **kw)
    with open(args.resolved, "wb") as f:  # (numpy.savez would append ".npz" to a bare name)
        numpy.savez(f, **{n: buffers[n].cpu().numpy() for n in names})
    return args.resolved


def write_ids(sc, args):
    """The ranked id-coverage buffers of the frame (or strip) as one .npz file: `ids` and `counts`
    int32 (H, W, K), `other` int32 (H, W), row 0 at the top; `samples`, the samples per pixel;
    `names`, the objects' (or the materials') names in index order."""
    key = args.id_key if args.id_key is not None else "object"
    kw = {}
    if args.subimage is not None and args.tasks is not None:
        kw = dict(subimage=args.subimage, tasks=args.tasks)
    buffers = sc.render_ids(args.id_ranks if args.id_ranks is not None else 4, key, ID_NAMES, **kw)
    named = sc.objects if key == "object" else sc.materials
    with open(args.ids, "wb") as f:  # (numpy.savez would append ".npz" to a bare name)
        numpy.savez(f, samples=numpy.int32(sc.samples_per_pixel), names=numpy.array([str(x.name) for x in named], dtype=str),
                    **{n: buffers[n].cpu().numpy() for n in ID_NAMES})
    return args.ids


def rgba_image(rgb, sc):
    """uint8 (H, W, 4): the frame's PNG bytes ``rgb`` with the coverage as A, converted on the
    device like the colour (rtx_fb_to_rgb8). Associated alpha: the colour already holds the
    misses' black."""
    from .scene import fb_to_rgb8
    a = fb_to_rgb8(sc.render_resolved(("alpha",))["alpha"]).cpu().numpy()
    return numpy.dstack([rgb, a])


def render_panorama(sc, width, height):
    """The panorama's PNG bytes, uint8 (height, width, 3): panorama_rays shaded at the camera's
    motion times, converted on the device like a render (rtx_fb_to_rgb8)."""
    import torch
    from .scene import fb_to_rgb8, panorama_rays
    o, d = panorama_rays(sc.vc, width, height)
    o, d = (torch.as_tensor(numpy.ascontiguousarray(a.T)).cuda() for a in (o, d))
    fb = sc.cast_rays_device(o, d, [float(t) for t in sc.vc.motion_times])
    return fb_to_rgb8(fb.view(height, width, 3)).cpu().numpy()


def _scene(args):
    from .scene_parser import load_scene
    if args.resolution is None and args.spp is None:
        return load_scene(args.infile, verbose=not args.quiet)
    with open(args.infile) as f:
        data = json.load(f)
    if args.resolution is not None:
        data["resolution"] = list(args.resolution)
    if args.spp is not None:
        data.setdefault("AA", {"jitter": False, "samples": 1})["samples"] = args.spp[0]
        if len(args.spp) > 1:
            data.setdefault("DOF", {"focal_length": 1, "aperture": 0, "samples": 1})["samples"] = args.spp[1]
    data["__base_dir__"] = os.path.dirname(os.path.abspath(args.infile))
    return load_scene(data, verbose=not args.quiet)


def main(argv=None):
    args = parse(argv)
    import torch
    from PIL import Image
    if args.distributed:
        import torch.distributed as dist
        from .distributed import render_frame
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        rank, world = dist.get_rank(), dist.get_world_size()
        sc = _scene(args)
        frame = render_frame(sc, rank, world, dtype=torch.uint8)
        if rank == 0:
            Image.fromarray(frame.cpu().numpy()).save(args.outfile)
        dist.destroy_process_group()
        return
    full_scene = _scene(args)
    if args.panorama is not None:
        Image.fromarray(render_panorama(full_scene, *args.panorama)).save(args.outfile)
        return
    if args.frames is not None:
        render_frames_to_files(full_scene, args)
        return
    if args.subimage is not None and args.tasks is not None:
        image = full_scene.render(args.subimage, args.tasks)
        numpy.save(args.outfile, image)
    else:
        rgb = full_scene.render_rgb8()  # == (rot90(render()) * 255).astype(uint8), on the device
        Image.fromarray(rgb).save(args.outfile)
        if args.rgba is not None:
            Image.fromarray(rgba_image(rgb, full_scene), "RGBA").save(args.rgba)
    if args.aovs is not None:
        write_aovs(full_scene, args)
    if args.occlusion is not None:
        write_occlusion(full_scene, args)
    if args.resolved is not None:
        write_resolved(full_scene, args)
    if args.ids is not None:
        write_ids(full_scene, args)


if __name__ == "__main__":
    main()
