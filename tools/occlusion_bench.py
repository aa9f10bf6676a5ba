#!/usr/bin/env python3
"""Time Scene.render_occlusion against the composition it replaces. Per scene,
at 1920x1080 and one sample per pixel, four variants, each a captured graph of repeated calls
timed with device events, replayed --rounds times in turn after a warm-up replay (the variants
alternate within a round):

  lights    render_occlusion("lights")
  ao        render_occlusion("ao"), K directions, unbounded rays
  both      render_occlusion(("lights", "ao"))
  composed  what a caller had to do for `ao` before the pass existed, through the existing API
            only: render_aovs(("position", "normal")), torch operations that build the frame
            and the n * K SoA rays (24 B each; the fp64 t_max array is built once, outside the
            timing), one rtx_occluded, and a torch reduction to the [H, W] buffer

Prints one JSON line per scene and variant (median, min and max us per call over the rounds)
and says whether the composed buffer equals the fused one bit for bit. Needs one MI355X.

    python tools/occlusion_bench.py [--out FILE.jsonl] [--calls 50] [--composed-calls 4] [--rounds 9]
"""
import argparse
import ctypes as C
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
from rtx import _native as N  # noqa: E402
from rtx.io import bundled_scene_dict  # noqa: E402

SCENES = ("TwoSpheresPlane", "TorusMesh")


def scene(name, res):
    d = bundled_scene_dict(name, resolution=res)
    d["AA"] = {"jitter": False, "samples": 1}
    return rtx.load_scene(d, verbose=False)


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


class Composed:
    """`ao` from render_aovs + torch + rtx_occluded; the frame is rtx.h's, one torch operation
    per fp32 operation (eager elementwise kernels do not fuse)."""

    def __init__(self, sc, dirs, out):
        self.sc, self.K, self.out = sc, int(dirs.shape[0]), out
        self.dirs = torch.as_tensor(dirs).cuda()
        self.n = out.numel()
        self.tmax = torch.full((self.n * self.K,), float("inf"), dtype=torch.float64, device="cuda")
        self.up = torch.tensor([0.0, 0.0, 1.0], device="cuda")
        self.time = float(sc.vc.motion_times[0])

    def __call__(self):
        K, n = self.K, self.n
        b = self.sc.render_aovs(("position", "normal"))
        p, nr = b["position"].view(n, 3), b["normal"].view(n, 3)
        miss = (nr == 0).all(dim=1)
        nr = torch.where(miss[:, None], self.up, nr)   # (a miss has no frame; its rays are discarded below)
        q = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        nh = nr * (1.0 / torch.sqrt(q))[:, None]
        x, y, z = nh.unbind(1)
        s = torch.copysign(torch.ones_like(z), z)
        a = -1.0 / (s + z)
        bb = (x * y) * a
        T = torch.stack([1.0 + ((s * x) * x) * a, s * bb, -(s * x)])   # [3, n]
        U = torch.stack([bb, s + ((y * y) * a), -y])
        dx, dy, dz = (self.dirs[:, c][None, None, :] for c in range(3))
        d = ((dx * T[:, :, None]) + (dy * U[:, :, None])) + (dz * nh.t()[:, :, None])   # [3, n, K]
        o = p.t()[:, :, None].expand(3, n, K).contiguous()
        occ = torch.empty(n * K, dtype=torch.uint8, device="cuda")
        vp = C.c_void_p
        N.call("rtx_occluded", self.sc.native().h, n * K, vp(o.data_ptr()), vp(d.data_ptr()), vp(self.tmax.data_ptr()),
               self.time, vp(occ.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
        free = K - occ.view(n, K).sum(dim=1, dtype=torch.int32)
        ao = free.to(torch.float32) / float(K)
        self.out.copy_(torch.where(miss, torch.ones_like(ao), ao).view(self.out.shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--composed-calls", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--ao-samples", type=int, default=16)
    ap.add_argument("--resolution", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--scenes", nargs="+", default=list(SCENES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.rounds >= 1 and args.calls >= 1 and args.composed_calls >= 1
    K = args.ao_samples
    dirs = rtx.cosine_directions(K)
    lines = []
    alive = []  # every scene lives to the end: destroying one frees device memory, which would break a capture
    for name in args.scenes:
        res = tuple(args.resolution)
        W, H = res
        sc = scene(name, res)
        li = torch.empty((H, W), dtype=torch.int32, device="cuda")
        ao = torch.empty((H, W), dtype=torch.float32, device="cuda")
        ao2 = torch.empty((H, W), dtype=torch.float32, device="cuda")
        sc.render_occlusion(ao_samples=K, out=dict(lights=li, ao=ao))
        composed = Composed(sc, dirs, ao2)
        variants = {
            "lights": (capture(lambda: sc.render_occlusion("lights", out=dict(lights=li)), args.calls), args.calls),
            "ao": (capture(lambda: sc.render_occlusion("ao", ao_samples=K, out=dict(ao=ao)), args.calls), args.calls),
            "both": (capture(lambda: sc.render_occlusion(ao_samples=K, out=dict(lights=li, ao=ao)), args.calls),
                     args.calls),
            "composed": (capture(composed, args.composed_calls), args.composed_calls),
        }
        torch.cuda.synchronize()
        same = bool(torch.equal(ao, ao2))
        differ = int((ao != ao2).sum().item())
        t = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v, (g, calls) in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                t[v].append(e0.elapsed_time(e1) * 1e3 / calls)
        for v, (_, calls) in variants.items():
            med = statistics.median(t[v])
            line = dict(scene=name, resolution=list(res), variant=v, ao_samples=K, calls=calls, rounds=args.rounds,
                        us_median=round(med, 3), us_min=round(min(t[v]), 3), us_max=round(max(t[v]), 3),
                        us_all=[round(x, 3) for x in t[v]], mean_ao=round(float(ao.mean().item()), 4),
                        lit_pixels=round(float((li != 0).float().mean().item()), 4))
            if v == "composed":
                line.update(equals_fused=same, pixels_differing=differ, ray_bytes=24 * W * H * K,
                            tmax_bytes=8 * W * H * K)
            lines.append(line)
            print(json.dumps(line), flush=True)
        alive.append((sc, variants, composed, li, ao, ao2))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
