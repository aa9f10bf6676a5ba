#!/usr/bin/env python3
"""Time Scene.cast_rays_device on the reference camera's own rays against render_device
(DESIGN.md §6ac). Per scene, at 1920x1080 and one sample per pixel, five variants, each a
captured graph of --calls calls timed with device events, replayed --rounds times in turn
(the variants alternate within a round):

  cast          cast_rays_device(camera_rays), coherent: ray i is pixel i
  cast_permuted the same rays in a seeded random order, group 1 (incoherent waves)
  generic_like  render_device, the generic kernel (option jit 0) without the camera-derived
                culling: bins, shadow_bins, self_skip and dsgrid 0 -- the same arithmetic as cast
  generic       render_device, the generic kernel with its defaults
  specialized   render_device, the scene-specialized kernel

Prints one JSON line per scene and variant (median, min and max us per call over the rounds,
the kernel's name for renders, input GB/s for the casts at 24 B per ray) and checks that cast
equals the render bit for bit. Needs one MI355X.

    python tools/cast_rays_bench.py [--out FILE.jsonl] [--calls 200] [--rounds 9]
    rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/cast_rays_bench.py --eager 20
"""
import argparse
import gc
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "python-raytracer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtx  # noqa: E402
from rtx.io import bundled_scene_dict  # noqa: E402

SCENES = ("TwoSpheresPlane", "MirrorRefraction", "TorusMesh")
LIKE = dict(bins="0", shadow_bins="0", self_skip="0", dsgrid="0")


def scene(name, res):
    d = bundled_scene_dict(name, resolution=res)
    d["AA"] = {"jitter": False, "samples": 1}
    return rtx.load_scene(d, verbose=False)


class Options:
    """Library options for the duration of a block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: rtx.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            rtx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            rtx.set_option(k, ("%d" % v) if isinstance(v, float) and v == int(v) else v)


def capture(fn, calls):
    """fn() run eagerly (warm-up, allocations), then `calls` times in one graph."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gc.collect()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--resolution", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--scenes", nargs="+", default=list(SCENES))
    ap.add_argument("--eager", type=int, default=0, metavar="N",
                    help="no graphs, no timing: N eager calls of each cast (under rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.rounds >= 1 and args.calls >= 1
    lines = []
    alive = []  # every scene lives to the end: destroying one frees device memory, which would break a capture
    for name in args.scenes:
        res = tuple(args.resolution)
        variants = {}  # name -> (graph, extra)
        keep = []      # scenes and tensors the graphs point into
        # the casts: rays of the reference camera, as they come and permuted
        sc = scene(name, res)
        o, d, group = sc.camera_rays(device=True)
        n = o.shape[1]
        times = [float(t) for t in sc.vc.motion_times]
        out = torch.empty((n // group, 3), dtype=torch.float32, device="cuda")
        perm = torch.as_tensor(np.random.RandomState(1).permutation(n)).cuda()
        op, dp = o[:, perm].contiguous(), d[:, perm].contiguous()
        outp = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        if args.eager:  # for a profiler: the two casts only, launched one by one
            for _ in range(args.eager):
                sc.cast_rays_device(o, d, times, group, out=out)
            for _ in range(args.eager):
                sc.cast_rays_device(op, dp, times, 1, out=outp)
            torch.cuda.synchronize()
            alive.append(sc)
            continue
        variants["cast"] = (capture(lambda: sc.cast_rays_device(o, d, times, group, out=out), args.calls), {})
        variants["cast_permuted"] = (capture(lambda: sc.cast_rays_device(op, dp, times, 1, out=outp), args.calls), {})
        keep += [sc, o, d, op, dp, out, outp]
        frames = {}
        for vname, opts in (("generic_like", dict(LIKE, jit="0")), ("generic", dict(jit="0")), ("specialized", {})):
            with Options(**opts):
                s2 = scene(name, res)
                fb = torch.empty((res[1], res[0], 3), dtype=torch.float32, device="cuda")
                s2.render_device(out=fb)
                s2.jit_wait()
                g = capture(lambda: s2.render_device(out=fb), args.calls)
                variants[vname] = (g, dict(kernel=s2.last_kernel))
            frames[vname] = fb
            keep += [s2, fb]
        torch.cuda.synchronize()
        same = all(torch.equal(out.view(res[1], res[0], 3), fb) for fb in frames.values())
        same_perm = bool(torch.equal(outp, out[perm])) if group == 1 else None
        t = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, (g, _) in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                t[v].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        for v, (_, extra) in variants.items():
            med = statistics.median(t[v])
            line = dict(scene=name, resolution=list(res), variant=v, rays=n, calls=args.calls, rounds=args.rounds,
                        us_median=round(med, 3), us_min=round(min(t[v]), 3), us_max=round(max(t[v]), 3),
                        us_all=[round(x, 3) for x in t[v]], equals_render=same, **extra)
            if v.startswith("cast"):
                line["input_GBps"] = round(24.0 * n / med / 1e3, 1)
                line["Mrays_per_s"] = round(n / med, 1)
            if v == "cast_permuted":
                line["equals_cast"] = same_perm
            lines.append(line)
            print(json.dumps(line), flush=True)
        alive.append((variants, keep))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    assert all(line["equals_render"] for line in lines), "cast_rays differs from the render"


if __name__ == "__main__":
    main()
