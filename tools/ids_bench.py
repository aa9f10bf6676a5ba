#!/usr/bin/env python3
"""Time Scene.render_ids beside the render_resolved passes it is built on. Per
scene, at 1920x1080, each variant is a captured graph of repeated calls timed with device events,
replayed --rounds times in turn after a warm-up replay (the variants alternate within a round):

  resolved_alpha        render_resolved(("alpha",))
  resolved_matte        render_resolved(("matte",), matte=[1]): one object set's matte, the pass
                        a compositor repeats per object without render_ids
  resolved_alpha_matte  render_resolved(("alpha", "matte"), matte=[1])
  ids_object_r4         render_ids(4, "object")
  ids_object_r8         render_ids(8, "object")
  ids_material_r4       render_ids(4, "material")

Flat scenes only (both passes refuse hierarchy/texture scenes). Prints one JSON line per scene and
variant (median, min and max us per call over the rounds; for the ids variants also the ratio of
the medians to resolved_alpha_matte and the break-even number of resolved_matte calls). Needs one
MI355X.

    python tools/ids_bench.py [--out FILE.jsonl] [--rounds 9] [--scenes NAME ...]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "python-raytracer_amd"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import rtx  # noqa: E402
from rtx.io import bundled_scene_dict  # noqa: E402
from resolved_bench import capture, time_variants  # noqa: E402


def crowd(d):
    """54 small spheres on a 9 x 6 grid before the DepthOfField bundle's plane, through a wide
    lens with 32 DOF origins: pixels with many objects (tests/test_gpu_ids.py's crowd case)."""
    d["AA"] = {"jitter": False, "samples": 1}
    d["DOF"] = {"aperture": 0.8, "focal_length": 3.0, "samples": 32}
    objects = [d["objects"][0]]
    for k in range(54):
        iy, ix = divmod(k, 9)
        objects.append({"type": "sphere", "name": "crowd%02d" % k, "radius": 0.13,
                        "position": [-1.2 + 0.3 * ix, 0.3 + 0.3 * iy, -1.5], "materials": [d["materials"][k % 3]["ID"]]})
    d["objects"] = objects
    return d


# name -> (bundled scene, edit of its dictionary, calls per graph)
SCENES = {
    "DepthOfField": ("DepthOfField", lambda d: d, 4),
    "MotionBlur": ("MotionBlur", lambda d: d, 10),
    "TwoSpheresPlane_aa4": ("TwoSpheresPlane", lambda d: dict(d, AA={"jitter": False, "samples": 4}), 20),
    "Crowd_dof32": ("DepthOfField", crowd, 4),
}


def scene(name, res):
    bundled, edit, calls = SCENES[name]
    return rtx.load_scene(edit(bundled_scene_dict(bundled, resolution=res)), verbose=False), calls


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
    for name in args.scenes:
        res = tuple(args.resolution)
        sc, calls = scene(name, res)
        fns = {
            "resolved_alpha": lambda: sc.render_resolved(("alpha",)),
            "resolved_matte": lambda: sc.render_resolved(("matte",), matte=[1]),
            "resolved_alpha_matte": lambda: sc.render_resolved(("alpha", "matte"), matte=[1]),
            "ids_object_r4": lambda: sc.render_ids(4, "object"),
            "ids_object_r8": lambda: sc.render_ids(8, "object"),
            "ids_material_r4": lambda: sc.render_ids(4, "material"),
        }
        variants = {v: (capture(fn, calls), calls) for v, fn in fns.items()}
        t = time_variants(variants, args.rounds)
        med = {v: statistics.median(t[v]) for v in variants}
        for v in variants:
            line = dict(scene=name, resolution=list(res), variant=v, samples=sc.samples_per_pixel, calls=calls,
                        rounds=args.rounds, us_median=round(med[v], 3), us_min=round(min(t[v]), 3),
                        us_max=round(max(t[v]), 3), us_all=[round(x, 3) for x in t[v]])
            if v.startswith("ids_"):
                line["over_resolved_alpha_matte"] = round(med[v] / med["resolved_alpha_matte"], 4)
                line["break_even_matte_calls"] = round(med[v] / med["resolved_matte"], 3)
            lines.append(line)
            print(json.dumps(line), flush=True)
        alive.append((sc, variants))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
