#!/usr/bin/env python3
"""Time Scene.render_resolved beside the passes around it. Per scene, at
1920x1080, each variant is a captured graph of repeated calls timed with device events,
replayed --rounds times in turn after a warm-up replay (the variants alternate within a round):

  resolved_ad     render_resolved(("alpha", "depth"))
  resolved_4      render_resolved(("alpha", "depth", "normal", "albedo"))
  resolved_5      the same plus "matte" (of object 1)
  aovs            render_aovs(), the six first-sample buffers
  render_generic  render_device() through the generic kernel (option jit 0)

Flat scenes only (the pass refuses hierarchy/texture scenes). Prints one JSON line per scene and
variant (median, min and max us per call over the rounds). Needs one MI355X.

    python tools/resolved_bench.py [--out FILE.jsonl] [--rounds 9] [--scenes NAME ...]
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

import torch  # noqa: E402

import rtx  # noqa: E402
from rtx.io import bundled_scene_dict  # noqa: E402

# name -> (bundled scene, edits, calls per graph)
SCENES = {
    "DepthOfField": ("DepthOfField", {}, 4),
    "MotionBlur": ("MotionBlur", {}, 10),
    "TwoSpheresPlane_aa4": ("TwoSpheresPlane", {"AA": {"jitter": False, "samples": 4}}, 20),
}


def scene(name, res):
    bundled, edits, calls = SCENES[name]
    d = bundled_scene_dict(bundled, resolution=res)
    d.update(edits)
    return rtx.load_scene(d, verbose=False), calls


def capture(fn, calls):
    """fn() run eagerly (warm-up, allocations), then `calls` times in one graph."""
    for _ in range(2):
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


def time_variants(variants, rounds):
    t = {v: [] for v in variants}
    for _ in range(rounds):
        for v, (g, calls) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            t[v].append(e0.elapsed_time(e1) * 1e3 / calls)
    return t


def report(lines, name, res, sc, variants, t, rounds, extra):
    for v, (_, calls) in variants.items():
        line = dict(scene=name, resolution=list(res), variant=v, samples=sc.samples_per_pixel, calls=calls,
                    rounds=rounds, us_median=round(statistics.median(t[v]), 3), us_min=round(min(t[v]), 3),
                    us_max=round(max(t[v]), 3), us_all=[round(x, 3) for x in t[v]])
        line.update(extra.get(v, {}))
        lines.append(line)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--resolution", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--scenes", nargs="*", default=list(SCENES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []
    alive = []  # every scene lives to the end: destroying one frees device memory, which would break a capture
    four = ("alpha", "depth", "normal", "albedo")
    for name in args.scenes:
        res = tuple(args.resolution)
        sc, calls = scene(name, res)
        variants = {
            "resolved_ad": (capture(lambda: sc.render_resolved(("alpha", "depth")), calls), calls),
            "resolved_4": (capture(lambda: sc.render_resolved(four), calls), calls),
            "resolved_5": (capture(lambda: sc.render_resolved(rtx.RESOLVED_NAMES, matte=[1]), calls), calls),
            "aovs": (capture(lambda: sc.render_aovs(), 20), 20),
        }
        rtx.set_option("jit", 0)
        variants["render_generic"] = (capture(lambda: sc.render_device(), calls), calls)
        kernels = {"render_generic": dict(kernel=sc.last_kernel)}
        rtx.set_option("jit", 1)
        report(lines, name, res, sc, variants, time_variants(variants, args.rounds), args.rounds, kernels)
        alive.append((sc, variants))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
