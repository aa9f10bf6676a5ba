// rtx_kernels.h — device side of the render path: per-frame parameters, the per-pixel
// sample loops (scene.py:47-79) and the kernels of librtx.so. Compiled into librtx.so
// (rtx_api.hip) and, for scene-specialized kernels, at run time by hiprtc (rtx_jit.cpp),
// which only needs render_body.
#pragma once

#include "rtx_trace.h"
#if defined(__HIPCC_RTC__)
#include "rtx.h"  // handed to hiprtc by name
#else
#include "../../include/rtx.h"
#endif

namespace rtx {

// The camera block: every wave-uniform value of the one-sample path at the head of KParams,
// contiguous and 64-byte aligned, so a one-sample scene-specialized kernel fetches it with a
// few wide scalar loads straight off the kernel argument, all issued together at the top of
// render_body (no pointer between the argument and the values: dof0 / aa0 are copies of
// dof_o[0] / aa_o[0], written by rtx_camera_set on every upload).
struct alignas(64) KParams {
    float pos[4], u[4], v[4], dw[4];
    float focal, divisor, jscale, inv_divisor;
    int32_t width, height, col0, ncols;
    float dof0[4], aa0[4];  // dof_o[0][0..2], aa_o[0][0][0..2]
    // RTX_PRIM_ORIGIN kernels (one sample, no jitter, static scene: every primary ray starts
    // at aa_o[0]): its origin-only plane and sphere terms, computed by rtx_camera_set with
    // closest_hit's fp32 operations (po_valid: computed)
    int32_t po_valid, pad_h0, pad_h1, pad_h2;
    float po_pnum[4];
    float po_sq[16];
    float po_soc[16][3];
    // (the end of the camera block)
    SceneView S;
    // camera tables (device)
    cptr<float> xs;
    cptr<float> ys;
    cptr<float> dof_o;   // [n_dof][3]
    cptr<float> aa_o;    // [n_dof][n_aa][3]
    cptr<float> times;   // [n_times] fp32; a sequence camera's [n_frames][n_times] (time_base)
    cptr<float> noise;   // replay jitter
    // n_frames: windows in `times` (host bookkeeping; the kernels index by Launch::tbase / tstep)
    int32_t div_pow2, n_frames, pad1, pad2;
    int32_t n_dof, n_aa, n_times, jitter;
    uint32_t seed_lo, seed_hi;
    // tools/wave_timeline.py only (kernels built with RTX_WAVE_LOG): per wave, its start
    // and end (s_memrealtime, 100 MHz) and hardware ids, 4 x uint64 per wave of the launch
    unsigned long long* wave_log;
    // measured tile schedule (RTX_TILE_SCHED kernels, rtx_api.hip tile_schedule): the
    // dispatch order of a whole frame's 8x8 tiles (wave w renders tile tile_perm[w]) and,
    // while it is measured, each tile's wave duration (s_memrealtime ticks); tile_n entries
    cptr<int32_t> tile_perm;
    unsigned int* tile_time;
    int32_t tile_n;
    // the camera's primary-ray direction table (ray_slot below; rtx_api.hip CamTables::rays):
    // primary_dir of every pixel of the strip, or null (the camera is outside the class)
    cptr<float> ray_dirs;
};

template <bool COUNT>
__device__ __forceinline__ void flush_tally(const Tally& tl, unsigned long long* counters, bool active) {
    if (!COUNT || counters == nullptr) return;
    uint32_t vals[RTX_COUNTERS] = {};
#pragma unroll
    for (int k = 0; k < kMaxDepth; ++k) vals[k] = active ? tl.cast[k] : 0u;
    vals[RTX_CNT_SHADOW] = active ? tl.shadow : 0u;
    vals[RTX_CNT_SHADE] = active ? tl.shade : 0u;
    vals[RTX_CNT_TRI] = active ? tl.tri : 0u;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < RTX_COUNTERS; ++k) {
        unsigned long long s = vals[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0 && s) atomicAdd(&counters[k], s);
    }
}

// Sample counts per pixel; the scene-specialized kernels pin them (with the camera's
// values) so the sample loops of the 1-spp configs disappear.
#ifdef RTX_FIXED_SAMPLES
#define RTX_NDOF(P) RTX_FIXED_NDOF
#define RTX_NAA(P) RTX_FIXED_NAA
#define RTX_NTIMES(P) RTX_FIXED_NTIMES
#else
#define RTX_NDOF(P) (P).n_dof
#define RTX_NAA(P) (P).n_aa
#define RTX_NTIMES(P) (P).n_times
#endif

// scene.py:54-55: base_ray_direction and focal_point of pixel (column cc, reference row j).
RTX_HD f3 pixel_focal(const KParams& P, int32_t cc, int j) {
    float fx = P.xs[cc];
    float fy = P.ys[j];
#if RTX_WAVE_HEAD  // both loads in flight before either is used
    asm volatile("" : "+v"(fx), "+v"(fy));
#endif
    // base_ray_direction = normalize(x * u + y * v - d * w)  (scene.py:54)
    const f3 bdir = normalize(sub(add(scale(ld3(P.u), fx), scale(ld3(P.v), fy)), ld3(P.dw)));
    return add(ld3(P.pos), scale(bdir, P.focal));  // scene.py:55
}

// scene.py:58: the direction of DOF sample kd's rays through pixel (column cc, reference row
// j), from that sample's lens origin toward the pixel's focal point. One-sample kernels take
// the origin from the camera block's copy.
RTX_HD f3 primary_dir(const KParams& P, int32_t cc, int j, int kd = 0) {
    const f3 focal = pixel_focal(P, cc, j);
#if RTX_WAVE_HEAD  // (one sample: the camera block's copy of dof_o[0])
    return normalize(sub(focal, ld3(P.dof0)));
#else
    return normalize(sub(focal, ld3(P.dof_o + 3 * kd)));
#endif
}

// The direction table of a one-sample, unjittered camera (KParams::ray_dirs): primary_dir
// depends on the camera and the pixel only, so rtx_camera_set computes it once per pixel
// (k_ray_dirs) and the scene-specialized kernels of such cameras (RTX_RAY_TABLE, rtx_api.hip
// jit_spec) read it instead of computing it in every frame. Three fp32 per pixel, tile-major:
// the slot of image row r (row 0 = top), strip column cc. An 8x8 tile on the 8-row grid is
// 768 contiguous bytes, one 12-byte load per lane; a tile off the grid (a row block with
// row0 % 8 != 0) reads parts of two. Ragged right and bottom tiles are allocated whole.
#ifndef RTX_RAY_TABLE
#define RTX_RAY_TABLE 0
#endif
RTX_HD uint32_t ray_slot(int32_t r, int32_t cc, int32_t ncols) {
    const uint32_t tiles_x = (uint32_t)(ncols + 7) >> 3;
    return (((uint32_t)r >> 3) * tiles_x + ((uint32_t)cc >> 3)) * 64u + ((uint32_t)r & 7u) * 8u + ((uint32_t)cc & 7u);
}
__host__ __device__ inline int64_t ray_table_slots(int32_t height, int32_t ncols) {
    return (int64_t)((height + 7) >> 3) * ((ncols + 7) >> 3) * 64;
}
// Slot s of the table (k_ray_dirs on the device, a loop in the host emulation). The slots of
// a ragged tile that lie outside the image take the nearest pixel's direction; no rendered
// pixel reads them.
RTX_HD f3 ray_table_entry(const KParams& P, int64_t s) {
    const int32_t tiles_x = (P.ncols + 7) >> 3;
    const int32_t tile = (int32_t)(s >> 6), lane = (int32_t)(s & 63);
    const int32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int32_t r = ty * 8 + (lane >> 3), cc = tx * 8 + (lane & 7);
    return primary_dir(P, cc < P.ncols ? cc : P.ncols - 1, P.height - 1 - (r < P.height ? r : P.height - 1));
}

#ifdef RTX_FIXED_JMODE  // scene-specialized kernels pin the jitter mode
#define RTX_JMODE(P) RTX_FIXED_JMODE
#else
#define RTX_JMODE(P) (P).jitter
#endif

// Production jitter (RTX_JITTER_PHILOX): sample s = kd * n_aa + ka of pixel (column
// col0 + cc, reference row j) takes half s & 1 of one Philox4x32-10 block with counter
// (col0 + cc, j, s >> 1, 0) and the scene's seed: 128 bits -> 6 uniforms of 21 bits,
// three per sample (half 0: the top 21 bits of words 0-2; half 1: their low 11 bits
// joined with 10-bit pieces of word 3). Consecutive samples share a block, so a pixel's
// samples cost half a Philox evaluation each (the render loops keep the block).
RTX_HD void jitter_block(const KParams& P, int32_t cc, int j, int pair, uint32_t w[4]) {
    w[0] = (uint32_t)(P.col0 + cc);
    w[1] = (uint32_t)j;
    w[2] = (uint32_t)pair;
    w[3] = 0u;
    philox4x32(w, P.seed_lo, P.seed_hi);
}
RTX_HD f3 jitter_rnd(const uint32_t w[4], int half) {
    const uint32_t a = half ? ((w[0] & 0x7FFu) | ((w[3] & 0x3FFu) << 11)) : w[0] >> 11;
    const uint32_t b = half ? ((w[1] & 0x7FFu) | (((w[3] >> 10) & 0x3FFu) << 11)) : w[1] >> 11;
    const uint32_t c = half ? ((w[2] & 0x7FFu) | (((w[3] >> 20) & 0x3FFu) << 11)) : w[2] >> 11;
    return mk((float)a * 0x1p-21f, (float)b * 0x1p-21f, (float)c * 0x1p-21f);
}

// scene.py:60-65: the origin of AA sample ka of DOF sample kd, jittered (JIT). jr: this
// sample's Philox uniforms when the caller has them (render_pixel keeps the odd sample's
// from the pair's block), else they are computed here.
template <bool JIT>
RTX_HD f3 sample_origin(const KParams& P, int32_t cc, int j, int kd, int ka, const f3* jr = nullptr) {
#if RTX_WAVE_HEAD  // (one sample: the camera block's copy of aa_o[0])
    f3 o = ld3(P.aa0);
#else
    f3 o = ld3(P.aa_o + 3 * (kd * RTX_NAA(P) + ka));
#endif
    if (JIT) {  // scene.py:63-65
        f3 rnd;
        if (RTX_JMODE(P) == RTX_JITTER_REPLAY) {
            const int64_t idx = (((int64_t)cc * P.height + j) * RTX_NDOF(P) + kd) * RTX_NAA(P) + ka;
            rnd = ld3(P.noise + 3 * idx);
        } else if (RTX_PROBE(15)) {  // cost probe only: no RNG
            rnd = mk(0.25f + 0.001f * (float)ka, 0.5f, 0.75f + 0.001f * (float)kd);
        } else if (jr != nullptr) {
            rnd = *jr;
        } else {
            const int s = kd * RTX_NAA(P) + ka;
            uint32_t w[4];
            jitter_block(P, cc, j, s >> 1, w);
            rnd = jitter_rnd(w, s & 1);
        }
        o = add(o, scale(normalize(rnd), P.jscale));
    }
    return o;
}

// colour / (samples * dof_samples * len(motion_times)) (scene.py:73); for a power of two
// the exact reciprocal multiply gives the identical correctly rounded result.
RTX_HD float sample_mean(const KParams& P, float c) {
#if defined(RTX_FIXED_SAMPLES) && RTX_FIXED_NDOF * RTX_FIXED_NAA * RTX_FIXED_NTIMES == 1
    (void)P;
    return c;  // one sample: the divisor is 1 and c * 1.0f is c, bit for bit (no load before the store)
#elif defined(RTX_FIXED_DIVPOW2)
    return RTX_FIXED_DIVPOW2 ? c * P.inv_divisor : c / P.divisor;
#else
    return P.div_pow2 ? c * P.inv_divisor : c / P.divisor;
#endif
}

// The framebuffer store. fp32 RGB (rtx_render), or -- scene-specialized kernels built
// with RTX_OUT8=1 for rtx_render_rgb8 -- main.py:33's (v * 255).astype(uint8) of the same
// fp32 value, written as bytes (the PNG's layout: 4x fewer bytes to store and to gather).
#ifndef RTX_OUT8
#define RTX_OUT8 0
#endif
// RTX_FB_GLOBAL (the kernels with a direction table, rtx_api.hip jit_spec): the fp32 store through
// a pointer typed as global memory. The framebuffer pointer loses its address space in
// pin_uniform64's integer round trip, so the store is otherwise a flat one.
#ifndef RTX_FB_GLOBAL
#define RTX_FB_GLOBAL 0
#endif
RTX_HD void put_channel(float* fb, int64_t i, float v) {
    if (RTX_OUT8)
        reinterpret_cast<uint8_t*>(fb)[i] = (uint8_t)(int)((double)v * 255.0);
#if RTX_FB_GLOBAL && defined(__HIP_DEVICE_COMPILE__)
    else
        ((__attribute__((address_space(1))) float*)fb)[i] = v;
#else
    else
        fb[i] = v;
#endif
}

// Multi-sample kernels re-read the scene records in every sample instead of keeping
// them live across the sample loops: the compiler otherwise hoists every record load and
// its loop-invariant VALU conversions (fp64 box bounds, padded culling boxes) out of the
// loops, where they occupy SGPRs and VGPRs for the kernel's whole life and spill (the
// DepthOfField kernel: 54 SGPRs into VGPR lanes and 176 B/lane of scratch, written once
// per pixel = 1.46 GB per 4K frame). Re-reads are scalar-cache hits, once per sample.
#ifndef RTX_RELOAD_RECORDS
#if defined(RTX_FIXED_SAMPLES)
#define RTX_RELOAD_RECORDS (RTX_FIXED_NDOF * RTX_FIXED_NAA * RTX_FIXED_NTIMES > 1)
#else
#define RTX_RELOAD_RECORDS 1
#endif
#endif
// A wave-uniform pointer the compiler cannot prove loop-invariant (its halves pass through
// readfirstlane, a no-op on a uniform value, and an empty asm that "redefines" them).
template <class T>
__device__ __forceinline__ cptr<T> opaque_uniform(cptr<T> p) {
    const uint64_t v = (uint64_t)p;
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    asm volatile("" : "+s"(lo), "+s"(hi));
    return (cptr<T>)(((uint64_t)hi << 32) | lo);
}
// (flat-scene kernels only: the hierarchy/texture kernels keep the loaded records)
//
// One-sample scene-specialized kernels built with RTX_BAKED_RECORDS carry the scene's object,
// material and light records in the code object (rtx_api.hip jit_baked_records: constant
// arrays rtx_baked::kObjs / kMats / kLights, defined ahead of this header). Reads at a
// compile-time index -- the unrolled object and light loops -- fold to literals, so no
// dependent scalar load precedes a wave's first ray; per-lane reads (the hit object, its
// material) load from the code object's read-only data. The values are the same bytes
// rtx_scene_create uploads, so the arithmetic is unchanged.
template <bool X>
RTX_HD SceneView sample_scene(const SceneView& S0) {
    SceneView S = S0;
#if defined(RTX_BAKED_RECORDS) && defined(__HIP_DEVICE_COMPILE__)
    if (!X) {
        S.objs = (cptr<DObj>)rtx_baked::kObjs;
        S.mats = (cptr<DMat>)rtx_baked::kMats;
        S.lights = (cptr<DLight>)rtx_baked::kLights;
        return S;
    }
#endif
#if defined(__HIP_DEVICE_COMPILE__)
    if (RTX_RELOAD_RECORDS && !X) {  // opaque to loop-invariant code motion
        S.objs = opaque_uniform(S.objs);
        if (RTX_RELOAD_RECORDS > 1) {
            S.mats = opaque_uniform(S.mats);
            S.lights = opaque_uniform(S.lights);
        }
    }
#endif
    return S;
}

// Tile classes (SceneView::bin_class; rtx_api.hip sb_bin proves them per camera). One-sample
// scene-specialized kernels of flat scenes of primary and shadow rays built with RTX_TILE_CLASS
// (rtx_api.hip jit_spec, option tile_class) read the tile's record where the others read its
// object mask and branch on the class word at once (render_body); the host emulation reads the
// same record in render_pixel. A tile of class UNSHADOWED takes render_pixel_plane, which stores
// what render_pixel stores for such a pixel and counts what it counts: closest_hit's test of
// plane 0 (valid in every lane and the only hit), then shade_uniform<0> with occ_mask 0 -- the
// operations of the general path on the same values, without the hit-object vote and without a
// shadow test. (SKY tiles take the general path: ending their waves at once measured 0.4-0.5 us
// slower on TwoSpheresPlane 1080p)
#ifndef RTX_TILE_CLASS
#define RTX_TILE_CLASS 0
#endif
template <bool COUNT>
RTX_HD void render_pixel_plane(const KParams& P, float* fb, int32_t ncols, int32_t rr, int32_t cc, f3 o, f3 d, float time,
                               Tally& tl, const HStack& hs) {
    const SceneView S = sample_scene<false>(P.S);
    if (COUNT) tl.cast[0]++;
    const DObj ob = S.objs[0];  // simple_geometry.py:105-120 (closest_hit's plane loop, k = 0)
    const f3 n = ld3(ob.b);
    const float denom = dot(d, n);
#if defined(RTX_PRIM_ORIGIN) && RTX_PRIM_ORIGIN && defined(RTX_FIXED_COUNTS)
    const float num = P.po_pnum[0];
#else
    const float num = dot(sub(moved(ob, ob.a, time), o), n);
#endif
    const Hit h{num / denom, 0, 0};
    HHit hh;  // (a hierarchy hit's record: never read for a plane)
    const f3 tail = clamp01(shade_uniform<false, COUNT, 0>(S, h, hh, o, d, time, tl, hs, -1, 0));
    const f3 colour = add(mk(0.0f, 0.0f, 0.0f), tail);
    const int64_t p = (int64_t)rr * ncols + cc;
    put_channel(fb, 3 * p, sample_mean(P, colour.x));
    put_channel(fb, 3 * p + 1, sample_mean(P, colour.y));
    put_channel(fb, 3 * p + 2, sample_mean(P, colour.z));
}

// scene.py:47-79 for pixel p of the output block (host/device: the tests-only host
// emulation runs the same body). tb: the index in P.times of the frame's window of motion
// times (time_base below; 0 for every camera without a sequence).
template <bool MESH, bool SEC, bool X, bool COUNT, bool JIT>
RTX_HD void render_pixel(const KParams& P, float* fb, int32_t row0, int32_t rr, int32_t cc, Tally& tl,
                         const FrameStack& fs, const HStack& hs, int32_t bin = -1, int32_t tb = 0,
                         const f3* tdir = nullptr) {
#ifdef RTX_FIXED_NCOLS  // (render_body's)
    const int32_t ncols = RTX_FIXED_NCOLS;
#else
    const int32_t ncols = P.ncols;
#endif
    if (RTX_PROBE(14)) {  // cost probe only: store a constant (launch + framebuffer write)
        const int64_t p = (int64_t)rr * ncols + cc;
        put_channel(fb, 3 * p, 0.5f); put_channel(fb, 3 * p + 1, 0.25f); put_channel(fb, 3 * p + 2, 0.125f);
        return;
    }
    const int j = P.height - 1 - (row0 + rr);  // reference row index (y grows upward)
    const int32_t blane = bin >= 0 ? (((row0 + rr) & 7) << 3) | (cc & 7) : -1;  // the pixel in its tile
#if !defined(__HIP_DEVICE_COMPILE__)
    // (the host emulation: the tile's class record, as an RTX_TILE_CLASS kernel's render_body reads it)
    if (!MESH && !SEC && !X && bin >= 0 && P.S.bin_class != nullptr && P.n_dof * P.n_aa * P.n_times == 1) {
        const uint32_t cls = P.S.bin_class[bin].y;
        if (cls & kTileUnshadowed) {
            const f3 d = P.ray_dirs != nullptr ? ld3(P.ray_dirs + 3 * (int64_t)ray_slot(row0 + rr, cc, ncols))
                                               : primary_dir(P, cc, j, 0);
            render_pixel_plane<COUNT>(P, fb, ncols, rr, cc, sample_origin<false>(P, cc, j, 0, 0), d, P.times[tb], tl, hs);
            return;
        }
    }
#endif
#if defined(RTX_PRIM_ORIGIN) && RTX_PRIM_ORIGIN && defined(RTX_FIXED_COUNTS)
    OriginTerms prim;  // the primary rays' origin-only terms (host-computed)
#pragma unroll
    for (int k = 0; k < RTX_FIXED_NP; ++k) prim.pnum[k] = P.po_pnum[k];
#pragma unroll
    for (int k = 0; k < RTX_FIXED_NS; ++k) {
        prim.soc[k] = ld3(P.po_soc[k]);
        prim.sq[k] = P.po_sq[k];
    }
    const OriginTerms* primp = &prim;
#else
    const OriginTerms* primp = nullptr;
#endif
    f3 colour = mk(0.0f, 0.0f, 0.0f);
    f3 jr_odd = mk(0.0f, 0.0f, 0.0f);  // the odd sample's jitter uniforms of the current pair
    // pinned counts must not unroll the loops (one cast_ray body per sample)
#pragma unroll 1
    for (int kd = 0; kd < RTX_NDOF(P); ++kd) {
        // the focal point is recomputed per DOF sample (the same fp32 operations) rather
        // than kept live across the loops (RTX_RELOAD_RECORDS)
        int32_t cc_k = cc, j_k = j;
#if defined(__HIP_DEVICE_COMPILE__)
        if (RTX_RELOAD_RECORDS) asm volatile("" : "+v"(cc_k), "+v"(j_k));
#endif
#if RTX_RAY_TABLE  // the pixel's table entry, which render_body read at the wave's start
        (void)cc_k; (void)j_k;
        const f3 ddir = *tdir;
#elif !defined(__HIP_DEVICE_COMPILE__)  // (the host emulation reads the camera's table, if it has one)
        (void)tdir;
        const f3 ddir = P.ray_dirs != nullptr ? ld3(P.ray_dirs + 3 * (int64_t)ray_slot(row0 + rr, cc, ncols))
                                              : primary_dir(P, cc_k, j_k, kd);  // scene.py:58
#else
        (void)tdir;
        const f3 ddir = primary_dir(P, cc_k, j_k, kd);  // scene.py:58
#endif
#pragma unroll 1
        for (int ka = 0; ka < RTX_NAA(P); ++ka) {
            // the Philox block of samples (2m, 2m + 1), computed at the even one; the odd
            // one's uniforms wait in jr
            const bool philox = JIT && RTX_JMODE(P) == RTX_JITTER_PHILOX && !RTX_PROBE(15);
            const bool odd = ((kd * RTX_NAA(P) + ka) & 1) != 0;
            f3 jr = jr_odd;
            if (philox && !odd) {
                uint32_t w[4];
                jitter_block(P, cc, j, (kd * RTX_NAA(P) + ka) >> 1, w);
                jr = jitter_rnd(w, 0);
                jr_odd = jitter_rnd(w, 1);
            }
            const f3 o = sample_origin<JIT>(P, cc, j, kd, ka, philox ? &jr : nullptr);
#pragma unroll 1
            for (int kt = 0; kt < RTX_NTIMES(P); ++kt)
                colour = add(colour, cast_ray<MESH, SEC, X, COUNT>(sample_scene<X>(P.S), o, ddir, P.times[tb + kt], tl, fs, hs,
                                                                   bin, primp, blane));
        }
    }
    colour = mk(sample_mean(P, colour.x), sample_mean(P, colour.y), sample_mean(P, colour.z));
#if RTX_PROBE_ON == 11 && defined(__HIP_DEVICE_COMPILE__)
    {  // cost probe only: RTX_PAD extra VALU instructions per pixel in 4 independent chains
        float c0 = colour.x, c1 = colour.y, c2 = colour.z, c3 = (float)cc;
#pragma unroll
        for (int k = 0; k < RTX_PAD / 4; ++k)
            asm volatile("v_add_f32 %0, %4, %0\n v_add_f32 %1, %4, %1\n v_add_f32 %2, %4, %2\n v_add_f32 %3, %4, %3"
                         : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3) : "v"((float)j));
        colour = mk(c0, c1, c2 + c3 * 0.0f);
    }
#endif
    const int64_t p = (int64_t)rr * ncols + cc;
    put_channel(fb, 3 * p, colour.x);
    put_channel(fb, 3 * p + 1, colour.y);
    put_channel(fb, 3 * p + 2, colour.z);
}

// Chunk c of a heavy tile's primary-ray face list (SceneView::bin_heavy): for the tile's
// pixel `lane` (row * 8 + column of its 8x8 tile), the closest of the chunk's faces by
// closest_hit's tests -- the face's padded box, then the exact test, offered to the same
// total order -- as (t32 bits, stored face or -1). The primary ray is render_pixel's of a
// one-sample pinhole camera (the bins' cameras): aa_o[0] toward the pixel's focal point.
// Every lane of a wave calls it for the same chunk (the loop's votes are the wave's).
// (Measured slower: starting chunks c >= 1 from chunk 0's closest face, in a second launch
// after it, blob 1080p 0.275 -> 0.291 ms; two faces per step, 0.201 -> 0.208-0.212 ms.)
RTX_HD uint2 mesh_chunk(const KParams& P, int32_t bin, int32_t c, int lane) {
    const SceneView& S = P.S;
    const int32_t ty = bin / S.bins_x, tx = bin - ty * S.bins_x;
    const int32_t row = ty * 8 + (lane >> 3), cc = tx * 8 + (lane & 7);
    const bool active = row < P.height && cc < P.ncols;
    const int j = P.height - 1 - (active ? row : 0);
    const f3 d = primary_dir(P, active ? cc : 0, j);  // scene.py:58
    const f3 o = ld3(P.aa_o);  // scene.py:60-61 (one sample, no jitter)
    const int32_t oi = S.n_plane + S.n_sphere + S.n_box;  // the scene's one top-level mesh
    const DObj ob = S.objs[oi];
    // (times[0] whatever the frame of a sequence: the chunks test the mesh, which does not move)
    const float time = P.times[0];
    const RayInv ri = ray_inv(o, d);
    Hit h{INFINITY, -1, 0};
    const int32_t q0 = S.bin_start[bin] + c * kHeavyChunk;
    const int32_t q1 = min(S.bin_start[bin + 1], q0 + kHeavyChunk);
    for (int32_t q = q0; q < q1; ++q) {
        if (RTX_ALL(!active || h.t32 < S.bin_zmin[q])) break;  // nearest first (closest_hit's exit)
        const int32_t f = S.bin_faces[q];
        const bool fmaybe = active && leaf_maybe_hit(RTX_FBOX(S, ob.tri_begin + f), o, ri, ob.cmax, h.t32);
        if (!RTX_ANY(fmaybe)) continue;
        float t32;
        const bool valid = tri_hit(RTX_TRI(S, ob.tri_begin + f), o, d, fmaybe, t32);
        offer(S, h, valid, t32, oi, f, o, d, time);
    }
    return make_uint2(__builtin_bit_cast(uint32_t, h.t32), h.obj >= 0 ? (uint32_t)h.sub : 0xFFFFFFFFu);
}

// mesh_chunk with the chunk's face records staged in LDS first (k_mesh_chunks mode bit 0,
// device only): one round of coalesced loads -- every lane fetches 16-byte words of the
// chunk's face records (its 32 face indices, then 96 B of triangle and 32 B of face box
// per face) -- instead of 2-3 dependent scalar loads per face inside the loop (the pass
// waited on memory 0.63 of its wave cycles, profiles/pmc_blob1080.json). The same tests,
// in the same order, as mesh_chunk.
#if defined(__HIP_DEVICE_COMPILE__)
struct ChunkLds {
    DTri tri[kHeavyChunk];
    DFaceBox box[kHeavyChunk];
    int32_t face[kHeavyChunk];
    float zmin[kHeavyChunk];
};
__device__ __forceinline__ uint2 mesh_chunk_lds(const KParams& P, int32_t bin, int32_t c, int lane, ChunkLds& sh) {
    const SceneView& S = P.S;
    const int32_t ty = bin / S.bins_x, tx = bin - ty * S.bins_x;
    const int32_t row = ty * 8 + (lane >> 3), cc = tx * 8 + (lane & 7);
    const bool active = row < P.height && cc < P.ncols;
    const int32_t oi = S.n_plane + S.n_sphere + S.n_box;  // the scene's one top-level mesh
    const DObj ob = S.objs[oi];
    const int32_t q0 = S.bin_start[bin] + c * kHeavyChunk;
    const int32_t n = min(S.bin_start[bin + 1], q0 + kHeavyChunk) - q0;
    if (lane < n) {
        sh.face[lane] = S.bin_faces[q0 + lane];
        sh.zmin[lane] = S.bin_zmin[q0 + lane];
    }
    __syncthreads();  // (one wave per block)
    constexpr int kTriW = (int)(sizeof(DTri) / 16), kBoxW = (int)(sizeof(DFaceBox) / 16), kW = kTriW + kBoxW;
    for (int w = lane; w < n * kW; w += 64) {
        const int i = w / kW, k = w - i * kW;
        const int64_t f = ob.tri_begin + sh.face[i];
        if (k < kTriW)
            reinterpret_cast<uint4*>(&sh.tri[i])[k] = reinterpret_cast<const uint4 RTX_CONST*>(&S.tris[f])[k];
        else
            reinterpret_cast<uint4*>(&sh.box[i])[k - kTriW] = reinterpret_cast<const uint4 RTX_CONST*>(&S.fboxes[f])[k - kTriW];
    }
    __syncthreads();
    const int j = P.height - 1 - (active ? row : 0);
    const f3 d = primary_dir(P, active ? cc : 0, j);  // scene.py:58
    const f3 o = ld3(P.aa_o);  // scene.py:60-61 (one sample, no jitter)
    const float time = P.times[0];  // (as mesh_chunk: static geometry)
    const RayInv ri = ray_inv(o, d);
    Hit h{INFINITY, -1, 0};
    for (int i = 0; i < n; ++i) {
        if (RTX_ALL(!active || h.t32 < sh.zmin[i])) break;  // nearest first (closest_hit's exit)
        const DFaceBox B = sh.box[i];
        const bool fmaybe = active && leaf_maybe_hit(B, o, ri, ob.cmax, h.t32);
        if (!RTX_ANY(fmaybe)) continue;
        float t32;
        const bool valid = tri_hit(sh.tri[i], o, d, fmaybe, t32);
        offer(S, h, valid, t32, oi, sh.face[i], o, d, time);
    }
    return make_uint2(__builtin_bit_cast(uint32_t, h.t32), h.obj >= 0 ? (uint32_t)h.sub : 0xFFFFFFFFu);
}
#endif

// Blocks of a split chunk to render again in the one-kernel form (rtx_split.h): n == nullptr
// for every other launch. A listed block's flag is set; the launch that renders it clears it.
struct RedoList {
    const uint32_t* n;       // blocks listed
    const uint32_t* blocks;  // their indices
    uint32_t* flags;         // per block of the chunk
};

// The per-frame parameters live in device memory (uploaded by rtx_camera_set) and are
// read with scalar loads; only the per-call output block is passed by value.
struct Launch {
    float* fb;
    unsigned long long* counters;
    int32_t row0, nrows;
    // gstride > 0 (rtx_render_groups): the block's rows are the 8-row groups gphase,
    // gphase + gstride, ... of the image, packed in order
    int32_t gphase, gstride;
    // rtx_render_frames: blockIdx.y renders frame y of a batch into fb + y * fstride bytes
    int64_t fstride;
    uint32_t perm;  // RTX_TILE_ORDER 2: the wave permutation's multiplier
    int32_t pix0;   // split hierarchy passes (rtx_split.h): the chunk's first pixel of the block
    int32_t tperm;  // RTX_TILE_SCHED kernels: 1 = dispatch a whole frame's tiles by P.tile_perm
    int32_t tlog;   // RTX_TILE_SCHED kernels: 1 = record each wave's duration in P.tile_time
    int32_t xcd;    // 1 = XCD-aware block order (xcd_block; tile-mapped render_body)
    // rtx_render_sequence: frame y of the launch (blockIdx.y) takes its motion times from
    // P.times[tbase + y * tstep + kt]. tstep = 0 (every other call): the frames are copies
    // of window tbase / n_times (rtx_render_frames); both 0 for a camera without a sequence.
    int32_t tbase, tstep;
    // render_body_spp as the split passes' fallback (rtx_split.h): render only the listed
    // blocks (chains that found the record pool full), pixels from pix0 on
    RedoList redo;
    // the current camera's per-pixel and per-tile tables (KParams::xs / ys, SceneView::
    // bin_objmask / bin_shadow), filled at launch: a one-sample scene-specialized kernel
    // addresses its tile's entries from the kernel arguments alone (render_body)
    cptr<float> xs, ys;
    cptr<uint32_t> bin_objmask, bin_shadow;
    cptr<float> ray_dirs;  // (KParams::ray_dirs)
    cptr<uint2> bin_class;  // (SceneView::bin_class)
    // SceneView::bins_x / bins_on of the current camera: a kernel with a direction table and no
    // tile schedule addresses its tile's record from the arguments alone and takes the bins'
    // grid from here, not from KParams. Every launcher of render_body fills them with the
    // tables above (render_launch, the only one).
    int32_t bins_x, bins_on;
};

// This block's framebuffer (frame blockIdx.y of a batched launch; the only frame otherwise).
__device__ __forceinline__ float* frame_fb(const Launch& L) {
    return reinterpret_cast<float*>(reinterpret_cast<char*>(L.fb) + (int64_t)blockIdx.y * L.fstride);
}

// The frame-dependent window of motion times (rtx_render_sequence). Scene-specialized
// kernels carry this arithmetic only when their camera holds a sequence (RTX_SEQUENCE=1 in
// their options): for every other camera they are what they were without it. The
// precompiled generic kernels take the run-time fields.
#ifndef RTX_SEQUENCE
#if defined(__HIPCC_RTC__)
#define RTX_SEQUENCE 0
#else
#define RTX_SEQUENCE 1
#endif
#endif

// Index in P.times of this block's window (host: Launch::tbase, one frame per call).
RTX_HD int32_t time_base(const Launch& L) {
#if RTX_SEQUENCE && defined(__HIP_DEVICE_COMPILE__)
    return L.tbase + (int32_t)blockIdx.y * L.tstep;
#elif RTX_SEQUENCE
    return L.tbase;
#else
    (void)L;
    return 0;
#endif
}

// Image row (row 0 = top) of block row rr.
__host__ __device__ inline int32_t image_row(const Launch& L, int32_t rr) {
    return L.gstride > 0 ? ((rr >> 3) * L.gstride + L.gphase) * 8 + (rr & 7) : L.row0 + rr;
}

// The primary-ray face bin of the 8x8 pixel tile whose top-left pixel is (image row,
// strip column, a multiple of 8), or -1 when the camera has no bins or the tile straddles
// two bin rows (row blocks that start off the 8-row grid).
// Scene-specialized kernels of cameras without bins are compiled with RTX_PRIMARY_BINS=0
// (the bin code vanishes); the precompiled kernels check bins_on at run time.
#ifndef RTX_PRIMARY_BINS
#define RTX_PRIMARY_BINS 1
#endif
__host__ __device__ inline int32_t primary_bin(const SceneView& S, int32_t row, int32_t col) {
    return RTX_PRIMARY_BINS && S.bins_on && (row & 7) == 0 ? (row >> 3) * S.bins_x + (col >> 3) : -1;
}

// Occupancy request (waves per SIMD) by kernel variant: mesh kernels without secondary
// rays fit 128 VGPRs without scratch and gain from 4 waves/SIMD; the flat primary+shadow
// kernels from 5 (DepthOfField 4K 11.2 -> 10.2 ms; TwoSpheresPlane already fits); the
// secondary-ray kernels lose if forced below their natural allocation (measured,
// tools/ablate.sh: 6 and 8 waves are slower everywhere).
#ifndef RTX_LB_WAVES
#define RTX_LB_WAVES(MESH, SEC) ((SEC) ? 1 : ((MESH) ? 4 : 5))
#endif
#ifndef RTX_TILE
#define RTX_TILE 1
#endif
// Pixels per lane: each wave renders RTX_PPL 8x8 tiles in sequence (amortises the
// per-wave setup chain: parameters, tables, scene records).
#ifndef RTX_PPL
#define RTX_PPL 1
#endif

// Output pixel (row, column within the block) of this work-item. RTX_TILE=1 maps each
// 64-lane wave to an 8x8 pixel tile (coherent rays per wave); 0 maps waves to 64
// consecutive pixels of a row. The wave's tile is wave-uniform, so its coordinates are
// scalar 32-bit arithmetic.
struct PixelRC {
    int32_t r, c;
};
// The order in which a launch's waves visit the tiles (experiments): 0 row-major from the
// top, 1 reversed (bottom rows first), 2 a stride permutation w -> w * perm mod T (the
// host picks perm coprime to the launch's T waves, near T / golden ratio), so each
// stretch of the dispatch samples the whole image.
#ifndef RTX_TILE_ORDER
#define RTX_TILE_ORDER 0
#endif
// Measured tile schedule (scene-specialized kernels of scenes with secondary rays or
// meshes, rtx_api.hip tile_schedule): whole-frame launches can dispatch the tiles in a
// table's order (longest measured first) and record each wave's duration.
#ifndef RTX_TILE_SCHED
#define RTX_TILE_SCHED 0
#endif
// XCD-aware block order (Launch::xcd, option xcd_map): the dispatcher hands workgroups to the 8 XCDs
// round-robin, so consecutive blocks -- neighbouring tiles, whose bin lists, tile-schedule
// entries and scene lines share cache lines -- would land in 8 different L2s. Block b
// instead takes slot block xcd_block(b): each XCD's k-th run of 16 waves (g blocks of
// 16/g waves) takes 16 consecutive tiles. Blocks of the last incomplete round of 8 runs keep
// their own index, so the map is a bijection on [0, nb). Host and device share it (the
// tile schedule's table is laid out through it, rtx_api.hip tile_schedule). Off by default:
// it cuts the fabric reads of the bins, light grids and schedule table (TorusMesh 1080p
// 29.8 -> 28.9 MB per frame, TwoSpheresPlane 26.2 -> 25.5, DepthOfField 4K 111.7 -> 109.5)
// but not the time (TwoSpheresPlane 22.06 -> 22.42 us, the 81,920-face mesh +1 %,
// DepthOfField -0.6 %; profiles/r05/xcd/).
__host__ __device__ inline uint32_t xcd_block(uint32_t b, uint32_t nb, uint32_t waves_per_block) {
    const uint32_t lg = waves_per_block >= 16 ? 0u : (waves_per_block >= 4 ? 2u : (waves_per_block >= 2 ? 3u : 4u));
    const uint32_t g = 1u << lg, round = 8u * g;
    if (b >= nb / round * round) return b;
    const uint32_t x = b & 7u, k = b >> 3;
    return (((k >> lg) << 3) + x) * g + (k & (g - 1u));
}
// B: the block size the kernel is launched with -- a constant of every kernel (kBlock), so
// no wave fetches it from the dispatch packet. The grid size, which comes from the implicit
// arguments (a scalar round trip at the start of every wave), is read only where its feature
// is compiled in: the tile orders 1 and 2, and the XCD map (RTX_XCD_MAP: the precompiled
// kernels, which take Launch::xcd at run time, and scene-specialized kernels compiled while
// option xcd_map is set).
#ifndef RTX_XCD_MAP
#if defined(RTX_FIXED_COUNTS)
#define RTX_XCD_MAP 0
#else
#define RTX_XCD_MAP 1
#endif
#endif
template <int B>
__device__ __forceinline__ PixelRC pixel_rc(int32_t ncols, int sub, uint32_t perm = 1, int32_t xcd = 0,
                                            const int32_t RTX_CONST* tperm = nullptr, int* tile = nullptr) {
    constexpr uint32_t W = B >> 6;  // waves per block
    const int lane = threadIdx.x & 63;
    uint32_t blk = blockIdx.x;
#if RTX_XCD_MAP
    if (xcd) blk = xcd_block(blockIdx.x, gridDim.x, W);
#endif
    int wave = __builtin_amdgcn_readfirstlane((int)((blk * W + (threadIdx.x >> 6)) * RTX_PPL + sub));
    if (RTX_TILE_SCHED && tperm != nullptr) wave = tperm[wave];
    if (tile) *tile = wave;
#if RTX_TILE_ORDER == 1 || RTX_TILE_ORDER == 2
    const uint32_t T = gridDim.x * W * RTX_PPL;
    if (RTX_TILE_ORDER == 1) wave = (int)T - 1 - wave;
    if (RTX_TILE_ORDER == 2) wave = (int)(((uint64_t)(uint32_t)wave * perm) % T);
#else
    (void)perm;
#endif
    if (RTX_TILE == 0) {
        const int64_t p = (int64_t)wave * 64 + lane;
        const int32_t r = (int32_t)(p / ncols);
        return PixelRC{r, (int32_t)(p - (int64_t)r * ncols)};
    }
    const int tiles_x = (ncols + 7) >> 3;
    const int ty = wave / tiles_x, tx = wave - ty * tiles_x;
    return PixelRC{ty * 8 + (lane >> 3), tx * 8 + (lane & 7)};
}

__host__ __device__ inline int64_t launch_items(int32_t nrows, int32_t ncols) {
    const int64_t waves = RTX_TILE == 0 ? ((int64_t)nrows * ncols + 63) / 64
                                        : (int64_t)((ncols + 7) >> 3) * ((nrows + 7) >> 3);
    return (waves + RTX_PPL - 1) / RTX_PPL * 64;
}

// Block size: 256 threads, or one wave for the hierarchy/texture (X) variants, whose
// per-thread ray/point stacks (9 words per hierarchy level) share the CU's LDS.
// 64 and 128 measured equal to 256 within noise with matching JIT kernels (library and
// hiprtc kernels both built with the value; tools/ab_block.sh, profiles/r02/blk: TSP
// 28.7/29.1/29.0 us, TM 83.0/82.1/81.9, MR 51.6/52.8/52.2, DOF 7.23/7.21/7.28 ms for
// 256/64/128)
#ifndef RTX_BLOCK_FLAT  // threads per block of the flat-scene kernels (experiments)
#define RTX_BLOCK_FLAT 256
#endif
template <bool X>
constexpr int kBlock = X ? 64 : RTX_BLOCK_FLAT;

// The body of k_render, shared with the scene-specialized kernels compiled at run time
// (rtx_jit.cpp), which pin the scene's object and light counts.
// RTX_LDS_TRIS kernels: the block copies the scene's triangles, face boxes and BVH nodes
// into LDS (16-byte words, all lanes) before tracing (rtx_trace.h RTX_TRI / RTX_LEAF).
__device__ __forceinline__ void stage_mesh_lds(const SceneView& S) {
#if defined(RTX_LDS_TRIS) && defined(__HIP_DEVICE_COMPILE__)
    auto copy = [](void* dst, const void RTX_CONST* src, int words) {
        uint4* d = static_cast<uint4*>(dst);
        const uint4 RTX_CONST* s = static_cast<const uint4 RTX_CONST*>(src);
        for (int i = threadIdx.x; i < words; i += blockDim.x) d[i] = s[i];
    };
    copy(g_lds_tris, S.tris, RTX_LDS_TRIS * (int)(sizeof(DTri) / 16));
    copy(g_lds_fboxes, S.fboxes, RTX_LDS_TRIS * (int)(sizeof(DFaceBox) / 16));
    copy(g_lds_leaves, S.leaves, RTX_LDS_LEAVES * (int)(sizeof(DLeaf) / 16));
    __syncthreads();
#else
    (void)S;
#endif
}

// RTX_LDS_OBJS kernels: the block copies the object and material records into LDS.
__device__ __forceinline__ void stage_records_lds(const SceneView& S) {
#if defined(RTX_LDS_OBJS) && defined(__HIP_DEVICE_COMPILE__)
    auto copy = [](void* dst, const void RTX_CONST* src, int words) {
        uint4* d = static_cast<uint4*>(dst);
        const uint4 RTX_CONST* s = static_cast<const uint4 RTX_CONST*>(src);
        for (int i = threadIdx.x; i < words; i += blockDim.x) d[i] = s[i];
    };
    copy(g_lds_objs, S.objs, RTX_LDS_OBJS * (int)(sizeof(DObj) / 16));
    copy(g_lds_mats, S.mats, RTX_LDS_MATS * (int)(sizeof(DMat) / 16));
    __syncthreads();
#else
    (void)S;
#endif
}

// Four wave-uniform words the compiler must hold in scalar registers from here on: their
// loads issue (and are waited for, once, with the others pinned beside them) where this
// stands instead of sinking, each into the basic block of its first use.
template <class T>
__device__ __forceinline__ void pin_uniform(T& a, T& b, T& c, T& d) {
    static_assert(sizeof(T) == 4, "32-bit scalars");
    uint32_t w0 = __builtin_bit_cast(uint32_t, a), w1 = __builtin_bit_cast(uint32_t, b);
    uint32_t w2 = __builtin_bit_cast(uint32_t, c), w3 = __builtin_bit_cast(uint32_t, d);
    asm volatile("" : "+s"(w0), "+s"(w1), "+s"(w2), "+s"(w3));
    a = __builtin_bit_cast(T, w0);
    b = __builtin_bit_cast(T, w1);
    c = __builtin_bit_cast(T, w2);
    d = __builtin_bit_cast(T, w3);
}

template <class T>  // (one of them)
__device__ __forceinline__ void pin_uniform(T& a) {
    static_assert(sizeof(T) == 4, "32-bit scalar");
    uint32_t w0 = __builtin_bit_cast(uint32_t, a);
    asm volatile("" : "+s"(w0));
    a = __builtin_bit_cast(T, w0);
}

template <class A, class B>  // (two wave-uniform pointers or 64-bit words)
__device__ __forceinline__ void pin_uniform64(A& a, B& b) {
    static_assert(sizeof(A) == 8 && sizeof(B) == 8, "64-bit scalars");
    uint64_t x = (uint64_t)a, y = (uint64_t)b;
    asm volatile("" : "+s"(x), "+s"(y));
    a = (A)x;
    b = (B)y;
}

// Wave timeline probe (experiment): the wave's start/end clock and where it ran.
#if defined(RTX_WAVE_LOG) && defined(__HIP_DEVICE_COMPILE__)
struct WaveClock {
    unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    __device__ void done(const KParams* Pp) const {
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        if ((threadIdx.x & 63) == 0 && Pp->wave_log != nullptr) {
            const uint64_t w = ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
            const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
            const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
            unsigned long long* o = Pp->wave_log + 4 * w;
            o[0] = t0;
            o[1] = t1;
            o[2] = hw;
            o[3] = xcc;
        }
    }
};
#define RTX_WAVE_CLOCK_BEGIN const WaveClock wclk_;
#define RTX_WAVE_CLOCK_END wclk_.done(Pp);
#else
#define RTX_WAVE_CLOCK_BEGIN
#define RTX_WAVE_CLOCK_END
#endif

template <bool MESH, bool SEC, bool X, bool COUNT, bool JIT>
__device__ __forceinline__ void render_body(const KParams* __restrict__ Pp, const Launch L0) {
    constexpr int B = kBlock<X>;
    RTX_WAVE_CLOCK_BEGIN
    if (MESH) stage_mesh_lds(Pp->S);
    stage_records_lds(Pp->S);
#ifdef RTX_FIXED_NCOLS  // scene-specialized kernels pin the strip width (tile index math by constants)
    const int32_t ncols = RTX_FIXED_NCOLS;
#else
    const int32_t ncols = Pp->ncols;
#endif
#if RTX_WAVE_HEAD
    // One-sample scene-specialized kernels: the frame parameters by value, read here, before
    // anything else, so every scalar load of the wave's prologue goes out off the kernel
    // arguments in one batch instead of one dependent round trip per use (each use sits in
    // its own basic block, behind the previous one's wait). What stood behind a pointer of
    // KParams comes from the camera block (dof0 / aa0: the only origins of a one-sample
    // camera) or is addressed from Launch's copies of the table pointers.
#if RTX_RAY_TABLE && !RTX_TILE_SCHED
    // A kernel with a direction table and no tile schedule knows its tile from its ids: what its
    // two table loads are addressed from -- the direction table, the tile records, the launch's
    // rows and the bins' grid (Launch's copies of SceneView's) -- is all of it kernel arguments,
    // pinned with the camera block's words, so every scalar load the path to the hit needs is
    // in flight before the wave's first scalar wait and the table loads issue behind that wait
    // (DESIGN.md 6ak). Kernels with a tile schedule learn their tile from a dependent load and
    // keep the form below, as do kernels without a table.
    static_assert(!X && RTX_TILE == 1 && RTX_PPL == 1, "one 8x8 tile per wave");
    Launch L = L0;
    KParams Q = *Pp;
    Q.S.bins_x = L.bins_x;
    Q.S.bins_on = L.bins_on;
    Q.xs = nullptr;  // (never read: the table stands for both)
    Q.ys = nullptr;
    Q.S.bin_objmask = L.bin_objmask;
    Q.S.bin_shadow = L.bin_shadow;
    pin_uniform64(L.ray_dirs, L.bin_class);
    pin_uniform(L.row0, L.nrows, L.gphase, L.gstride);
    // (The table stands for the camera's basis as well: pos, u, v, dw, focal and dof0 are never
    // read and not pinned. Groups are pinned whole, pad words included: a word of a load in
    // flight that nothing reads is a register the next load may be given, and that load then
    // waits for the first.)
    pin_uniform(Q.aa0[0], Q.aa0[1], Q.aa0[2], Q.aa0[3]);
    pin_uniform(Q.S.ambient[0], Q.S.ambient[1], Q.S.ambient[2], Q.S.ambient[3]);
    pin_uniform(Q.height, Q.S.bins_x, Q.S.bins_on, Q.ncols);
#if defined(RTX_PRIM_ORIGIN) && RTX_PRIM_ORIGIN && defined(RTX_FIXED_COUNTS)
    // (the hit tests' origin-only terms: render_pixel and render_pixel_plane read them)
#pragma unroll
    for (int k = 0; k < RTX_FIXED_NP; ++k) pin_uniform(Q.po_pnum[k]);
#pragma unroll
    for (int k = 0; k < RTX_FIXED_NS; ++k) pin_uniform(Q.po_soc[k][0], Q.po_soc[k][1], Q.po_soc[k][2], Q.po_sq[k]);
#endif
    pin_uniform64(Q.S.bin_objmask, Q.S.bin_shadow);
    float* fbp = frame_fb(L);
    int64_t fbw = L.fstride;  // (pinned beside it only)
    pin_uniform64(fbp, fbw);
    // The pixel's direction from the camera's table. The row is held inside the launch's rows:
    // lanes below a ragged bottom edge, and waves past the last tile, read an entry of the
    // last row (the columns of a ragged right tile have slots of their own).
    const cptr<float> tdirs = L.ray_dirs;
    auto table_dir = [&](const PixelRC& px) {
        const int32_t rq = px.r < L.nrows ? px.r : L.nrows - 1;
        return ld3(tdirs + 3u * ray_slot(image_row(L, rq), px.c, ncols));
    };
    f3 tdir = mk(0.0f, 0.0f, 0.0f);
    const PixelRC px_early = pixel_rc<B>(ncols, 0, L.perm, L.xcd);
    tdir = table_dir(px_early);
#if RTX_TILE_CLASS
    static_assert(!MESH && !SEC && !X && RTX_TILE == 1 && RTX_PPL == 1, "tile classes: flat primary + shadow kernels");
    const cptr<uint2> bclass = L.bin_class;
#endif
#else
    const Launch& L = L0;
    KParams Q = *Pp;
#if RTX_RAY_TABLE
    // The pixel's direction from the camera's table: its address needs the kernel arguments
    // and the wave's ids only, so the load goes out ahead of the wait for the camera block
    // (behind it measured 0.25 us slower). The row is held inside the launch's rows:
    // lanes below a ragged bottom edge, and waves past the last tile, read an entry of the
    // last row (the columns of a ragged right tile have slots of their own). A kernel with a
    // tile schedule knows its tile only after the permutation's entry (below).
    static_assert(RTX_TILE == 1 && RTX_PPL == 1, "one 8x8 tile per wave");
    const cptr<float> tdirs = L.ray_dirs;
    auto table_dir = [&](const PixelRC& px) {
        const int32_t rq = px.r < L.nrows ? px.r : L.nrows - 1;
        return ld3(tdirs + 3u * ray_slot(image_row(L, rq), px.c, ncols));
    };
    f3 tdir = mk(0.0f, 0.0f, 0.0f);
#if !RTX_TILE_SCHED
    const PixelRC px_early = pixel_rc<B>(ncols, 0, L.perm, L.xcd);
    tdir = table_dir(px_early);
#endif
    Q.xs = nullptr;  // (never read: the table stands for both)
    Q.ys = nullptr;
#else
    Q.xs = L.xs;
    Q.ys = L.ys;
#endif
    Q.S.bin_objmask = L.bin_objmask;
    Q.S.bin_shadow = L.bin_shadow;
#if RTX_TILE_CLASS
    static_assert(!MESH && !SEC && !X && RTX_TILE == 1 && RTX_PPL == 1, "tile classes: flat primary + shadow kernels");
    cptr<uint2> bclass = L.bin_class;
    int64_t bclass_pad = 0;  // (pinned beside it only)
    pin_uniform64(bclass, bclass_pad);
#endif
    if (!X) {
        pin_uniform(Q.pos[0], Q.pos[1], Q.pos[2], Q.focal);
        pin_uniform(Q.u[0], Q.u[1], Q.u[2], Q.dof0[0]);
        pin_uniform(Q.v[0], Q.v[1], Q.v[2], Q.dof0[1]);
        pin_uniform(Q.dw[0], Q.dw[1], Q.dw[2], Q.dof0[2]);
        pin_uniform(Q.aa0[0], Q.aa0[1], Q.aa0[2], Q.S.ambient[0]);
        pin_uniform(Q.height, Q.S.bins_x, Q.S.bins_on, Q.ncols);
#if !RTX_RAY_TABLE
        pin_uniform64(Q.xs, Q.ys);
#endif
        pin_uniform64(Q.S.bin_objmask, Q.S.bin_shadow);
    }
    float* fbp = frame_fb(L);
    int64_t fbw = L.fstride;  // (pinned beside it only)
    if (!X) pin_uniform64(fbp, fbw);
#endif
    const KParams& P = X ? *Pp : Q;  // (the hierarchy / texture kernels keep the pointer)
#else
    const Launch& L = L0;
    const KParams& P = *Pp;
    float* const fbp = frame_fb(L);
#endif
    Tally tl = {};
    // secondary-ray frames: [frame][word][thread] in LDS (40 KB per 256-thread block; 30 KB
    // with RTX_FRAME_MATBITS)
    __shared__ float frames[SEC ? kFrameLds * kFrameWords * B : 1];
    extern __shared__ float hstack[];  // X: [level][9][thread] (dynamic size)
    const FrameStack fs{frames + threadIdx.x, B};
    const HStack hs{hstack + threadIdx.x, B};
    bool any_active = false;
    const int32_t tb = time_base(L);
#if RTX_TILE_SCHED && defined(__HIP_DEVICE_COMPILE__)
    static_assert(RTX_TILE == 1 && RTX_PPL == 1, "the tile schedule orders whole 8x8 tiles");
    const unsigned long long tclk0 = L.tlog ? __builtin_amdgcn_s_memrealtime() : 0ull;
    int tile = 0;
#endif
    for (int sub = 0; sub < RTX_PPL; ++sub) {
#if RTX_TILE_SCHED && defined(__HIP_DEVICE_COMPILE__)
        const PixelRC px = pixel_rc<B>(ncols, sub, L.perm, L.xcd, L.tperm ? Pp->tile_perm : nullptr, &tile);
#elif RTX_WAVE_HEAD && RTX_RAY_TABLE
        const PixelRC px = px_early;
#else
        const PixelRC px = pixel_rc<B>(ncols, sub, L.perm, L.xcd);
#endif
#if RTX_WAVE_HEAD && RTX_RAY_TABLE && RTX_TILE_SCHED
        tdir = table_dir(px);
#endif
        const bool active = px.r < L.nrows && px.c < ncols;
        any_active = any_active || active;
        // primary-ray face bin of the wave's 8x8 tile (its top-left pixel)
        const int32_t bin = RTX_TILE == 1 ? primary_bin(P.S, image_row(L, px.r & ~7), px.c & ~7) : -1;
#if RTX_TILE_CLASS && RTX_WAVE_HEAD && RTX_PRIMARY_BINS
        // the tile's record: its object mask, as below, and its class word in the same scalar
        // load. The class is branched on at once, by scalar branches: nothing of it stays live
        // across the general path's hit test.
        // The load is one 64-bit word at an address that is valid whatever bin is (entry 0 for a
        // tile off the grid: a kernel with classes has a table), so it goes out here, beside the
        // direction table's, not behind the branch on bin and the wait for the direction.
        uint64_t rec = reinterpret_cast<cptr<uint64_t>>(bclass)[wave_uniform(bin >= 0 ? bin : 0)];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(rec));  // (pinned here: left to itself the load sinks to its use, below that wait)
#endif
        if (bin >= 0) {
            const uint32_t cls = (uint32_t)(rec >> 32);
            Q.S.tile_objmask = (uint32_t)rec;
            if (cls & kTileUnshadowed) {
                if (active) {
                    const int32_t row0c = image_row(L, px.r) - px.r;
#if RTX_RAY_TABLE
                    const f3 dc = tdir;
#else
                    const f3 dc = primary_dir(P, px.c, P.height - 1 - (row0c + px.r), 0);
#endif
                    render_pixel_plane<COUNT>(P, fbp, ncols, px.r, px.c,
                                              sample_origin<false>(P, px.c, P.height - 1 - (row0c + px.r), 0, 0), dc,
                                              P.times[tb], tl, hs);
                }
                continue;
            }
        }
#elif RTX_WAVE_HEAD && RTX_TILE == 1 && RTX_PRIMARY_BINS
        // the tile's object mask, fetched here and handed down by value (SceneView::tile_objmask)
        if (!X && bin >= 0) Q.S.tile_objmask = Q.S.bin_objmask[wave_uniform(bin)];
#endif
        // render_pixel's image row is row0 + rr: pass the image row of px.r as that sum
#if RTX_WAVE_HEAD && RTX_RAY_TABLE
        if (active)
            render_pixel<MESH, SEC, X, COUNT, JIT>(P, fbp, image_row(L, px.r) - px.r, px.r, px.c, tl, fs, hs, bin,
                                                   tb, &tdir);
#else
        if (active)
            render_pixel<MESH, SEC, X, COUNT, JIT>(P, fbp, image_row(L, px.r) - px.r, px.r, px.c, tl, fs, hs, bin,
                                                   tb);
#endif
    }
    flush_tally<COUNT>(tl, L.counters, any_active);
#if RTX_TILE_SCHED && defined(__HIP_DEVICE_COMPILE__)
    if (L.tlog && (threadIdx.x & 63) == 0 && tile < Pp->tile_n)
        Pp->tile_time[tile] = (unsigned int)(__builtin_amdgcn_s_memrealtime() - tclk0);
#endif
    RTX_WAVE_CLOCK_END
}

// n / d and n % d for 0 <= n < 2^22, d >= 1 (rd = fl32(1 / d)): the fp32 quotient is
// off by at most one, which the remainder test corrects. Full-rate 24-bit multiplies.
__device__ __forceinline__ int udiv_small(int n, int d, float rd, int& rem) {
    int q = (int)((float)n * rd);
    int r = n - (int)__umul24((unsigned)q, (unsigned)d);
    if (r >= d) { ++q; r -= d; }
    if (r < 0) { --q; r += d; }
    rem = r;
    return q;
}

// Pixels per block of the sample-parallel mapping (host and device agree on it).
__host__ __device__ inline int spp_pixels_per_block(int spp, int block) { return spp >= block ? 1 : block / spp; }

// Sample-parallel mapping for high sample counts (rtx_render picks it for the hierarchy /
// texture kernels when a pixel has >= RTX_SPP_MIN samples): the B lanes of a block trace the samples of P = B / spp
// consecutive pixels (row-major within the output block), or the samples of one pixel
// in ceil(spp / B) rounds, so a wave's rays start from one pixel (coherent) and a wave
// lasts one sample instead of all of them. Each lane puts its sample's colour in LDS;
// per (pixel, channel) one owner lane then adds them in the reference's order
// (dof, aa, time; scene.py:57-70) starting from +0 -- the same fp32 sums as
// render_pixel -- and writes the mean. Samples s map to (kd, ka, kt) with kt fastest.
template <bool MESH, bool SEC, bool X, bool COUNT, bool JIT>
__device__ __forceinline__ void render_block_spp(const KParams* __restrict__ Pp, const Launch& L, int64_t blk, Tally& tl,
                                                 bool& any_active) {
    constexpr int B = kBlock<X>;
    const KParams& P = *Pp;
    const int32_t ncols = P.ncols;
    const int nt = RTX_NTIMES(P), na = RTX_NAA(P);
    const int S = RTX_NDOF(P) * na * nt;
    const int PPB = spp_pixels_per_block(S, B);
    const int rounds = (PPB * S + B - 1) / B;
    const float rS = 1.0f / (float)S, rT = 1.0f / (float)nt, rA = 1.0f / (float)na;
    __shared__ float frames[SEC ? kFrameLds * kFrameWords * B : 1];
    __shared__ float sbuf[3 * B];
    extern __shared__ float hstack[];  // X: [level][9][thread] (dynamic size)
    const FrameStack fs{frames + threadIdx.x, B};
    const HStack hs{hstack + threadIdx.x, B};
    const int64_t npix = (int64_t)L.nrows * ncols;
    const int64_t pix0 = L.pix0 + blk * PPB;
    const int tid = threadIdx.x;
    const int32_t tb = time_base(L);
    float acc = 0.0f;  // rounds > 1 (one pixel per block): lane ch < 3 sums channel ch
    for (int rd = 0; rd < rounds; ++rd) {
        const int flat = rd * B + tid;  // the block's sample index
        int s;
        const int lp = udiv_small(flat, S, rS, s);
        const int64_t p = pix0 + lp;
        const bool active = lp < PPB && p < npix;
        f3 c = mk(0.0f, 0.0f, 0.0f);
        if (active) {
            any_active = true;
            const int32_t rr = (int32_t)(p / ncols), cc = (int32_t)(p - (int64_t)rr * ncols);
            const int j = P.height - 1 - image_row(L, rr);
            int kt, ka;
            const int da = udiv_small(s, nt, rT, kt);
            const int kd = udiv_small(da, na, rA, ka);
            const f3 ddir = primary_dir(P, cc, j, kd);  // scene.py:58
            const f3 o = sample_origin<JIT>(P, cc, j, kd, ka);
            c = cast_ray<MESH, SEC, X, COUNT>(P.S, o, ddir, P.times[tb + kt], tl, fs, hs);
        }
        sbuf[tid] = c.x;
        sbuf[B + tid] = c.y;
        sbuf[2 * B + tid] = c.z;
        __syncthreads();
        if (rounds == 1) {  // (pixel, channel) pairs, each summed in order by one lane
            for (int q = tid; q < 3 * PPB; q += B) {
                const int pp = q / 3, ch = q - 3 * (q / 3);
                if (pix0 + pp < npix) {
                    const float* src = sbuf + ch * B + pp * S;
                    float a = 0.0f;
                    for (int k = 0; k < S; ++k) a += src[k];
                    put_channel(frame_fb(L), 3 * (pix0 + pp) + ch, sample_mean(P, a));
                }
            }
        } else if (tid < 3) {  // this round's samples of the block's pixel
            const int hi = min(S - rd * B, B);
            const float* src = sbuf + tid * B;
            for (int k = 0; k < hi; ++k) acc += src[k];
        }
        __syncthreads();  // sbuf is reused by the next round (or block)
    }
    if (rounds > 1 && tid < 3 && pix0 < npix) put_channel(frame_fb(L), 3 * pix0 + tid, sample_mean(P, acc));
}

template <bool MESH, bool SEC, bool X, bool COUNT, bool JIT>
__device__ __forceinline__ void render_body_spp(const KParams* __restrict__ Pp, const Launch L) {
    Tally tl = {};
    bool any_active = false;
    // one block, or (the split passes' redo list) the grid strides over the listed blocks;
    // one call site either way
    const bool listed = L.redo.n != nullptr;
    const uint32_t nb = listed ? *L.redo.n : 1u;
    for (uint32_t i = listed ? blockIdx.x : 0u; i < nb; i += listed ? gridDim.x : 1u) {
        const uint32_t b = listed ? L.redo.blocks[i] : blockIdx.x;
        render_block_spp<MESH, SEC, X, COUNT, JIT>(Pp, L, (int64_t)b, tl, any_active);
        if (listed && threadIdx.x == 0) L.redo.flags[b] = 0u;
    }
    flush_tally<COUNT>(tl, L.counters, any_active);
}

#ifndef RTX_LB_XWAVES  // hierarchy/texture kernels: waves per SIMD requested (experiments)
#define RTX_LB_XWAVES 1
#endif
#define RTX_RENDER_BOUNDS(MESH, SEC, X) __launch_bounds__(rtx::kBlock<X>, (X) ? RTX_LB_XWAVES : RTX_LB_WAVES(MESH, SEC))

#if !defined(__HIPCC_RTC__)
template <bool MESH, bool SEC, bool X, bool COUNT, bool JIT>
__global__ RTX_RENDER_BOUNDS(MESH, SEC, X) void k_render(const KParams* __restrict__ Pp, const Launch L) {
    render_body<MESH, SEC, X, COUNT, JIT>(Pp, L);
}

template <bool MESH, bool SEC, bool X, bool COUNT, bool JIT>
__global__ RTX_RENDER_BOUNDS(MESH, SEC, X) void k_render_spp(const KParams* __restrict__ Pp, const Launch L) {
    render_body_spp<MESH, SEC, X, COUNT, JIT>(Pp, L);
}

// Ray i of n caller-built rays: origins and directions as SoA fp32 [3][n] (rtx_intersect's layout).
struct Ray {
    f3 o, d;
};
__device__ __forceinline__ Ray soa_ray(const float* ro, const float* rd, int64_t n, int64_t i) {
    return Ray{mk(ro[i], ro[n + i], ro[2 * n + i]), mk(rd[i], rd[n + i], rd[2 * n + i])};
}

// The public object id of a hit (-1: a miss; hier: a hierarchy hit, whose sub holds the id).
__device__ __forceinline__ int32_t hit_oid(const SceneView& S, const Hit& h, bool hier) {
    return h.obj == -1 ? -1 : hier ? h.sub : S.objs[h.obj].oid;
}

// The fp64 ray parameter of a hit (+inf: a miss).
__device__ __forceinline__ double hit_time64(const SceneView& S, const Hit& h, const HHit& hh, f3 o, f3 d, float time) {
    return h.obj == -1 ? (double)INFINITY : h.obj == kHierHit ? hh.t64 : hit_t64(S, h.obj, h.sub, o, d, time);
}

template <bool MESH, bool X>
__global__ __launch_bounds__(256) void k_intersect(SceneView S, int64_t n, const float* __restrict__ ro,
                                                   const float* __restrict__ rd, float time, double* t_out,
                                                   int32_t* obj_out, int32_t* mat_out, float* n_out, float* p_out) {
    extern __shared__ float hstack[];
    const HStack hs{hstack + threadIdx.x, (int)blockDim.x};
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Ray r = soa_ray(ro, rd, n, i);
    const f3 o = r.o, d = r.d;
    Tally tl = {};
    HHit hh;
    const Hit h = closest_hit<MESH, X, false>(S, o, d, time, tl, hs, hh);
    int32_t mat = -1;
    f3 nn = mk(0.0f, 0.0f, 0.0f), pp = mk(0.0f, 0.0f, 0.0f);
    const bool hit = h.obj != -1;
    if (hit) {
        const Surface sf = resolve_hit<MESH, X>(S, h, hh, o, d, time);
        mat = sf.mat;
        nn = sf.normal;
        pp = sf.position;
    }
    if (t_out) t_out[i] = hit_time64(S, h, hh, o, d, time);
    if (obj_out) obj_out[i] = hit_oid(S, h, h.obj == kHierHit);
    if (mat_out) mat_out[i] = mat;
    if (n_out) { n_out[i] = nn.x; n_out[n + i] = nn.y; n_out[2 * n + i] = nn.z; }
    if (p_out) { p_out[i] = pp.x; p_out[n + i] = pp.y; p_out[2 * n + i] = pp.z; }
}

template <bool MESH, bool X>
__global__ __launch_bounds__(256) void k_occluded(SceneView S, int64_t n, const float* __restrict__ ro,
                                                  const float* __restrict__ rd, const double* __restrict__ tmax,
                                                  float time, uint8_t* occ) {
    extern __shared__ float hstack[];
    const HStack hs{hstack + threadIdx.x, (int)blockDim.x};
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Ray r = soa_ray(ro, rd, n, i);
    const f3 o = r.o, d = r.d;
    Tally tl = {};
    occ[i] = occluded<MESH, X, false>(S, o, d, tmax[i], time, tl, hs) ? 1 : 0;
}

// The first hit of a lane's pixel (k_aov, k_occlusion). render_body's mapping over rows [row0,
// row0 + nrows) of the strip: one lane per pixel, an 8x8 tile per wave, the tile's primary bin
// under render_body's condition. The ray is the one of DOF origin 0, AA origin 0 with that
// sample's jitter draw (scene.py:57-65), at the motion time P.times[tbase]. closest_hit gets
// no pixel-in-tile (blane -1): a heavy mesh tile walks its face list, since only a render
// fills SceneView::mesh_hits. Two steps, so that a ragged-edge lane leaves by a plain return
// in the kernel before closest_hit's wave votes (one call with the exit inside it made the
// compiler merge the two paths and branch again): first_pixel gives px and in, the kernel
// returns on !in, first_hit fills in the rest.
struct FirstHit {
    PixelRC px;
    bool in;
    int32_t bin;
    f3 o, d;
    float time;
    Hit h;
    HHit hh;
};

template <bool X>
__device__ __forceinline__ FirstHit first_pixel(const KParams& P, int32_t nrows) {
    FirstHit f;
    const int32_t ncols = P.ncols;
    f.px = pixel_rc<kBlock<X>>(ncols, 0);
    f.in = f.px.r < nrows && f.px.c < ncols;
    return f;
}

template <bool MESH, bool X, bool JIT>
__device__ __forceinline__ void first_hit(const KParams& P, int32_t row0, int32_t tbase, const HStack& hs, Tally& tl,
                                          FirstHit& f) {
    f.bin = RTX_TILE == 1 ? primary_bin(P.S, row0 + (f.px.r & ~7), f.px.c & ~7) : -1;
    const int j = P.height - 1 - (row0 + f.px.r);  // reference row index (y grows upward)
    f.o = sample_origin<JIT>(P, f.px.c, j, 0, 0);
    f.d = primary_dir(P, f.px.c, j);  // scene.py:58
    f.time = P.times[tbase];
    f.h = closest_hit<MESH, X, false>(P.S, f.o, f.d, f.time, tl, hs, f.hh, f.bin, nullptr, -1);
}

// The per-call block of the first-hit pass (rtx_render_aov): rows [row0, row0 + nrows) of
// the strip, the frame's first motion time P.times[tbase], and one pointer per buffer
// (pixel-major like the framebuffer, [nrows][ncols] or [nrows][ncols][3]; null: not wanted).
struct AovLaunch {
    float* depth;
    float* normal;
    float* position;
    float* albedo;
    int32_t* object;
    int32_t* material;
    int32_t row0, nrows, tbase, pad;
};

RTX_HD void put3(float* out, int64_t p, f3 v) {
    out[3 * p] = v.x;
    out[3 * p + 1] = v.y;
    out[3 * p + 2] = v.z;
}

// What the first sample of each pixel sees (no reference counterpart: the attributes of
// scene.py:86-94's first_intersect for first_hit's ray at the frame's first motion time). A
// tile row's 8 pixels are one contiguous segment of every buffer (32 B, or 96 B for a vector).
template <bool MESH, bool X, bool JIT>
__global__ __launch_bounds__(kBlock<X>) void k_aov(const KParams* __restrict__ Pp, const AovLaunch L) {
    extern __shared__ float hstack[];  // X: [level][9][thread] (dynamic size)
    const HStack hs{hstack + threadIdx.x, kBlock<X>};
    const KParams& P = *Pp;
    const int32_t ncols = P.ncols;
    Tally tl = {};
    FirstHit f = first_pixel<X>(P, L.nrows);
    if (!f.in) return;
    first_hit<MESH, X, JIT>(P, L.row0, L.tbase, hs, tl, f);
    const Hit& h = f.h;
    const bool hit = h.obj != -1;
    const bool hier = X && h.obj == kHierHit;
    Surface sf;
    sf.position = mk(0.0f, 0.0f, 0.0f);
    sf.normal = mk(0.0f, 0.0f, 0.0f);
    sf.mat = -1;
    sf.gobj = -1;
    if (hit) sf = resolve_hit<MESH, X>(P.S, h, f.hh, f.o, f.d, f.time);
    const int64_t p = (int64_t)f.px.r * ncols + f.px.c;
    if (L.depth) L.depth[p] = !hit ? INFINITY : hier ? (float)f.hh.t64 : h.t32;
    if (L.position) put3(L.position, p, sf.position);
    if (L.normal) put3(L.normal, p, sf.normal);
    if (L.object) L.object[p] = hit_oid(P.S, h, hier);
    if (L.material) L.material[p] = sf.mat;
    if (L.albedo) {  // scene.py:143-146: Plane/AABB hits shade with get_diffuse(position)
        f3 a = mk(0.0f, 0.0f, 0.0f);
        if (hit)
            a = (X && sf.gobj >= 0) ? get_diffuse(P.S, P.S.objs[sf.gobj], sf.position, f.time)
                                    : ld3(RTX_MAT(P.S, sf.mat).diffuse);
        put3(L.albedo, p, a);
    }
}

// The per-call block of the occlusion pass (rtx_render_occlusion): rows [row0, row0 + nrows)
// of the strip, the frame's first motion time P.times[tbase], one pointer per buffer
// ([nrows][ncols]; null: not wanted) and the ambient-occlusion rays by value: n_dirs local
// directions (x, y along the tangents, z along the normal) and their t_max.
struct OccLaunch {
    uint32_t* lights;
    float* ao;
    int32_t row0, nrows, tbase, n_dirs;
    double radius;
    float dirs[RTX_AO_MAX_DIRS][3];
};

// Visibility at the first hit of each pixel (no reference counterpart). The ray, the hit, the
// motion time and the mapping are k_aov's: both call first_hit. From the hit's position p and
// normal n (the values k_aov stores):
//   lights  bit li = light li's shadow ray from p is free (scene.py:150-167, skip == False).
//           The tests are regular_lighting's level-0 calls of occluded, argument for argument
//           (the light's index, the hit's flat object, the tile's shadow-bin word), so they use
//           what a render's use: light grids, shadow bins, plane self tests, directional
//           shadow grids -- all built for the camera's own hit points, which p is.
//   ao      the share of n_dirs rays from p that are free up to t_max = radius; ray k runs
//           along x_k T + y_k U + z_k n^ in the branchless orthonormal frame of n^ =
//           normalize(n) (unfused fp32 in the order written below). These are not camera or
//           light rays: they go through occluded with its defaults (light -1, self_obj -1,
//           every object), which reads none of the camera's or the lights' tables.
// A miss stores 0 and 1.0. Lanes that missed sit out both loops (as in cast_ray, which
// leaves before regular_lighting): occluded's wave votes count active lanes only.
template <bool MESH, bool X, bool JIT>
__global__ __launch_bounds__(kBlock<X>) void k_occlusion(const KParams* __restrict__ Pp, const OccLaunch L) {
    extern __shared__ float hstack[];  // X: [level][9][thread] (dynamic size)
    const HStack hs{hstack + threadIdx.x, kBlock<X>};
    const KParams& P = *Pp;
    const int32_t ncols = P.ncols;
    Tally tl = {};
    FirstHit f = first_pixel<X>(P, L.nrows);
    if (!f.in) return;
    first_hit<MESH, X, JIT>(P, L.row0, L.tbase, hs, tl, f);
    const int32_t bin = f.bin;
    const float time = f.time;
    uint32_t lit = 0u;
    float open = 1.0f;
    if (f.h.obj != -1) {
        const Surface sf = resolve_hit<MESH, X>(P.S, f.h, f.hh, f.o, f.d, time);
        if (L.lights != nullptr) {
            cptr<uint32_t> sbm = nullptr;  // the tile's shadow bins (regular_lighting's)
            if (RTX_SHADOW_BINS && bin >= 0 && P.S.bin_shadow != nullptr)  // (wave-uniform)
                sbm = P.S.bin_shadow + (int64_t)wave_uniform(bin) * P.S.n_lights;
            for (int li = 0; li < P.S.n_lights; ++li) {
                const DLight Lt = P.S.lights[li];
                const bool point = Lt.type == LIGHT_POINT;
                const f3 sdir = point ? sub(ld3(Lt.vec), sf.position) : ld3(Lt.negvec);
                const double t_max = point ? 1.0 : (double)INFINITY;
                if (!occluded<MESH, X, false>(P.S, sf.position, sdir, t_max, time, tl, hs, nullptr, li, f.h.obj,
                                              sbm ? sbm[li] : ~0u))
                    lit |= 1u << li;
            }
        }
        if (L.ao != nullptr) {
            const f3 n = normalize(sf.normal);
            const float s = __builtin_copysignf(1.0f, n.z);
            const float a = -1.0f / (s + n.z);
            const float b = (n.x * n.y) * a;
            const f3 T = mk(1.0f + ((s * n.x) * n.x) * a, s * b, -(s * n.x));
            const f3 U = mk(b, s + ((n.y * n.y) * a), -n.y);
            int32_t free_rays = 0;
            for (int k = 0; k < L.n_dirs; ++k) {
                const f3 dk = add(add(scale(T, L.dirs[k][0]), scale(U, L.dirs[k][1])), scale(n, L.dirs[k][2]));
                if (!occluded<MESH, X, false>(P.S, sf.position, dk, L.radius, time, tl, hs)) ++free_rays;
            }
            open = (float)free_rays / (float)L.n_dirs;
        }
    }
    const int64_t p = (int64_t)f.px.r * ncols + f.px.c;
    if (L.lights != nullptr) L.lights[p] = lit;
    if (L.ao != nullptr) L.ao[p] = open;
}

// The per-call block of the resolved pass (rtx_render_resolved): rows [row0, row0 + nrows) of
// the strip, the window of motion times P.times[tbase .. tbase + n_times), one pointer per
// buffer ([nrows][ncols] or [nrows][ncols][3]; null: not wanted) and the matte set by value,
// bit i = top-level object i belongs to it.
struct ResolvedLaunch {
    float* alpha;
    float* matte;
    float* depth;
    float* normal;
    float* albedo;
    int32_t row0, nrows, tbase, pad;
    uint32_t matte_set[RTX_MATTE_MAX_OBJECTS / 32];
};

// What a pixel covers, over all its samples (no reference counterpart): render_pixel's sample
// loops (scene.py:57-69: DOF origins, AA origins, motion times, time fastest; the same rays and
// jitter draws, the odd sample's uniforms kept from its pair's Philox block) with the first
// hit's attributes summed where render_pixel sums the colour. The mapping is k_aov's, and so
// are closest_hit's arguments (the tile's primary bin, no pixel-in-tile). With S samples, H of
// them hits and M of those on an object of the matte set:
//   alpha   fl32(H) / fl32(S)         matte   fl32(M) / fl32(S)
//   depth   sum of k_aov's depth over the hits / fl32(H); +inf when H == 0
//   normal, albedo   sum of k_aov's normal / albedo over the hits / fl32(S): a miss adds
//           nothing, so they carry the coverage like the colour, whose misses add black
// Every sum is fp32 from +0 in sample order, every quotient one correctly rounded division.
// The surface is resolved only for normal and albedo (depth and the object come from the hit
// record), the albedo looked up only when wanted; the sums stay in registers and each buffer
// is stored once, a tile row as one contiguous 32 B or 96 B segment. A flat-scene kernel:
// no hierarchy stack, no textured albedo; rtx_render_resolved refuses hierarchy/texture scenes.
template <bool MESH, bool JIT>
__global__ __launch_bounds__(kBlock<false>) void k_resolved(const KParams* __restrict__ Pp, const ResolvedLaunch L) {
    const HStack hs{nullptr, kBlock<false>};  // (flat scenes: closest_hit never touches it)
    const KParams& P = *Pp;
    const int32_t ncols = P.ncols;
    Tally tl = {};
    const FirstHit f = first_pixel<false>(P, L.nrows);
    if (!f.in) return;
    const int32_t rr = f.px.r, cc = f.px.c;
    const int32_t bin = RTX_TILE == 1 ? primary_bin(P.S, L.row0 + (rr & ~7), cc & ~7) : -1;
    const int j = P.height - 1 - (L.row0 + rr);  // reference row index (y grows upward)
    const bool want_surface = L.normal != nullptr || L.albedo != nullptr;
    int32_t nhit = 0, nmatte = 0;
    float depth = 0.0f;
    f3 normal = mk(0.0f, 0.0f, 0.0f), albedo = mk(0.0f, 0.0f, 0.0f);
    f3 jr_odd = mk(0.0f, 0.0f, 0.0f);  // the odd sample's jitter uniforms of the current pair
    const int n_dof = P.n_dof, n_aa = P.n_aa, n_times = P.n_times;
#pragma unroll 1
    for (int kd = 0; kd < n_dof; ++kd) {
        // (the focal point is recomputed per DOF sample, not kept live: render_pixel's reason)
        int32_t cc_k = cc, j_k = j;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(cc_k), "+v"(j_k));
#endif
        const f3 ddir = primary_dir(P, cc_k, j_k, kd);  // scene.py:58
#pragma unroll 1
        for (int ka = 0; ka < n_aa; ++ka) {
            const bool philox = JIT && P.jitter == RTX_JITTER_PHILOX;
            const bool odd = ((kd * n_aa + ka) & 1) != 0;
            f3 jr = jr_odd;
            if (philox && !odd) {
                uint32_t w[4];
                jitter_block(P, cc, j, (kd * n_aa + ka) >> 1, w);
                jr = jitter_rnd(w, 0);
                jr_odd = jitter_rnd(w, 1);
            }
            // (two calls, each with a constant pointer: a selected one keeps jr in scratch)
            const f3 o = philox ? sample_origin<JIT>(P, cc, j, kd, ka, &jr) : sample_origin<JIT>(P, cc, j, kd, ka);
#pragma unroll 1
            for (int kt = 0; kt < n_times; ++kt) {
                const float time = P.times[L.tbase + kt];
                const SceneView S = sample_scene<false>(P.S);
                HHit hh;  // (hierarchy hits only: never filled here)
                const Hit h = closest_hit<MESH, false, false>(S, o, ddir, time, tl, hs, hh, bin, nullptr, -1);
                if (h.obj != -1) {  // (a miss adds nothing)
                    ++nhit;
                    if (L.matte != nullptr) {
                        const uint32_t oid = (uint32_t)hit_oid(S, h, false);
                        if (oid < (uint32_t)RTX_MATTE_MAX_OBJECTS && ((L.matte_set[oid >> 5] >> (oid & 31u)) & 1u))
                            ++nmatte;
                    }
                    if (L.depth != nullptr) depth += h.t32;
                    if (want_surface) {
                        const Surface sf = resolve_hit<MESH, false>(S, h, hh, o, ddir, time);
                        normal = add(normal, sf.normal);
                        if (L.albedo != nullptr) albedo = add(albedo, ld3(RTX_MAT(S, sf.mat).diffuse));
                    }
                }
            }
        }
    }
    const float ns = (float)(n_dof * n_aa * n_times);
    const int64_t p = (int64_t)rr * ncols + cc;
    if (L.alpha) L.alpha[p] = (float)nhit / ns;
    if (L.matte) L.matte[p] = (float)nmatte / ns;
    if (L.depth) L.depth[p] = nhit == 0 ? INFINITY : depth / (float)nhit;
    if (L.normal) put3(L.normal, p, mk(normal.x / ns, normal.y / ns, normal.z / ns));
    if (L.albedo) put3(L.albedo, p, mk(albedo.x / ns, albedo.y / ns, albedo.z / ns));
}

// The per-call block of the id pass (rtx_render_ids): rows [row0, row0 + nrows) of the strip,
// the window of motion times P.times[tbase .. tbase + n_times), one pointer per buffer (ids and
// counts [nrows][ncols][ranks], other [nrows][ncols]; null: not wanted) and the ranks written.
struct IdsLaunch {
    int32_t* ids;
    int32_t* counts;
    int32_t* other;
    int32_t row0, nrows, tbase, ranks;
};

// A pixel's id table: RTX_ID_SLOTS (key, count) pairs, an empty slot (-1, 0). Every index below
// is a compile-time constant after unrolling, so the sixteen words are registers.
struct IdTable {
    int32_t key[RTX_ID_SLOTS];
    int32_t cnt[RTX_ID_SLOTS];
};

// n >= 0 hit samples with key k (n == 0: nothing happens, whatever k is): the slot that holds
// k counts them; else the lowest empty slot becomes (k, n); else they are dropped (the kernel
// finds the dropped ones as its hit count less the slots' counts). The filled slots are a
// prefix, so the lowest empty one is slot `fill`. The slot selects sit behind a branch that a
// wave takes only while one of its lanes brings a new key.
__device__ __forceinline__ void id_add(IdTable& t, int32_t& fill, int32_t k, int32_t n) {
    bool found = n == 0;
#pragma unroll
    for (int i = 0; i < RTX_ID_SLOTS; ++i) {
        const bool held = t.key[i] == k;
        t.cnt[i] += held ? n : 0;
        found |= held;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    if (__builtin_amdgcn_ballot_w64(!found) == 0) return;  // (wave-uniform)
#endif
    const int32_t at = found ? -1 : fill;  // the slot a new key takes (RTX_ID_SLOTS: none left)
#pragma unroll
    for (int i = 0; i < RTX_ID_SLOTS; ++i) {
        const bool take = at == i;
        t.key[i] = take ? k : t.key[i];
        t.cnt[i] = take ? n : t.cnt[i];
    }
    fill += (!found && fill < RTX_ID_SLOTS) ? 1 : 0;
}

// The hit samples of a pixel reach its table as runs of equal keys: consecutive samples mostly
// see the same object, so a sample costs a compare and a count, and the table is touched only
// when a lane of the wave changes its key (a wave-uniform branch) and once at the end. Runs are
// added in sample order, which keeps the table's rule -- the first RTX_ID_SLOTS distinct keys --
// as it is stated per sample; a miss neither ends nor extends a run.
struct IdRun {
    int32_t key = -1, n = 0;
};

__device__ __forceinline__ void id_count(IdTable& t, int32_t& fill, IdRun& run, int32_t k) {
    const bool same = k == run.key;
    run.n += same ? 1 : 0;
#if defined(__HIP_DEVICE_COMPILE__)
    if (__builtin_amdgcn_ballot_w64(!same) == 0) return;  // (wave-uniform)
#endif
    id_add(t, fill, run.key, same ? 0 : run.n);  // (the lanes that go on with their run add nothing)
    run.key = k;
    run.n = same ? run.n : 1;
}

// Compare-exchange of slots A and B for the ranking: count descending, equal counts by key
// ascending, empty slots (count 0) last. One unsigned 64-bit compare of (count, ~key).
template <int A, int B>
__device__ __forceinline__ void id_exchange(IdTable& t) {
    const uint64_t a = ((uint64_t)(uint32_t)t.cnt[A] << 32) | (uint32_t)~t.key[A];
    const uint64_t b = ((uint64_t)(uint32_t)t.cnt[B] << 32) | (uint32_t)~t.key[B];
    const bool sw = a < b;
    const int32_t ka = t.key[A], ca = t.cnt[A];
    t.key[A] = sw ? t.key[B] : ka;
    t.cnt[A] = sw ? t.cnt[B] : ca;
    t.key[B] = sw ? ka : t.key[B];
    t.cnt[B] = sw ? ca : t.cnt[B];
}

// The eight slots in rank order: a 19-exchange, 6-layer sorting network.
__device__ __forceinline__ void id_rank(IdTable& t) {
    id_exchange<0, 2>(t); id_exchange<1, 3>(t); id_exchange<4, 6>(t); id_exchange<5, 7>(t);
    id_exchange<0, 4>(t); id_exchange<1, 5>(t); id_exchange<2, 6>(t); id_exchange<3, 7>(t);
    id_exchange<0, 1>(t); id_exchange<2, 3>(t); id_exchange<4, 5>(t); id_exchange<6, 7>(t);
    id_exchange<2, 4>(t); id_exchange<3, 5>(t);
    id_exchange<1, 4>(t); id_exchange<3, 6>(t);
    id_exchange<1, 2>(t); id_exchange<3, 4>(t); id_exchange<5, 6>(t);
}

// A lane's `ranks` words of one buffer, a contiguous run: 16-byte stores when the run is 4 or
// 8 words and the buffer is 16-byte aligned (`wide`, wave-uniform), single words otherwise.
__device__ __forceinline__ void id_store(int32_t* out, int64_t p, int32_t ranks, bool wide,
                                         const int32_t (&v)[RTX_ID_SLOTS]) {
    static_assert(RTX_ID_SLOTS == 8, "the run is stored as one or two 16-byte words");
    int32_t* const run = out + p * ranks;
    if (wide && ranks == 8) {
        reinterpret_cast<int4*>(run)[0] = make_int4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<int4*>(run)[1] = make_int4(v[4], v[5], v[6], v[7]);
    } else if (wide && ranks == 4) {
        reinterpret_cast<int4*>(run)[0] = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int r = 0; r < RTX_ID_SLOTS; ++r)
            if (r < ranks) run[r] = v[r];
    }
}

// Which objects (MAT false: hit_oid, rtx_render_aov's `object`) or materials (MAT true:
// resolve_hit's mat, its `material`) cover a pixel, over all its samples (no reference
// counterpart). The samples, rays, jitter draws, mapping and closest_hit arguments are
// k_resolved's, loop for loop. Each hit sample's key goes into the lane's IdTable, which keeps
// the first RTX_ID_SLOTS distinct keys in sample order with exact counts; later keys are only
// counted as dropped. After the last sample the slots are ranked and the first L.ranks of them
// stored: ids (-1: an empty rank), counts (0), and other = the hits not in a written rank, so
// sum(counts) + other is k_resolved's hit count H. The surface is resolved only for the
// material key. A flat-scene kernel, as k_resolved is.
template <bool MESH, bool JIT, bool MAT>
__global__ __launch_bounds__(kBlock<false>) void k_ids(const KParams* __restrict__ Pp, const IdsLaunch L) {
    const HStack hs{nullptr, kBlock<false>};  // (flat scenes: closest_hit never touches it)
    const KParams& P = *Pp;
    const int32_t ncols = P.ncols;
    Tally tl = {};
    const FirstHit f = first_pixel<false>(P, L.nrows);
    if (!f.in) return;
    const int32_t rr = f.px.r, cc = f.px.c;
    const int32_t bin = RTX_TILE == 1 ? primary_bin(P.S, L.row0 + (rr & ~7), cc & ~7) : -1;
    const int j = P.height - 1 - (L.row0 + rr);  // reference row index (y grows upward)
    IdTable t;
#pragma unroll
    for (int i = 0; i < RTX_ID_SLOTS; ++i) {
        t.key[i] = -1;
        t.cnt[i] = 0;
    }
    int32_t nhit = 0, fill = 0;
    IdRun run;
    f3 jr_odd = mk(0.0f, 0.0f, 0.0f);  // the odd sample's jitter uniforms of the current pair
    const int n_dof = P.n_dof, n_aa = P.n_aa, n_times = P.n_times;
#pragma unroll 1
    for (int kd = 0; kd < n_dof; ++kd) {
        // (the focal point is recomputed per DOF sample, not kept live: render_pixel's reason)
        int32_t cc_k = cc, j_k = j;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(cc_k), "+v"(j_k));
#endif
        const f3 ddir = primary_dir(P, cc_k, j_k, kd);  // scene.py:58
#pragma unroll 1
        for (int ka = 0; ka < n_aa; ++ka) {
            const bool philox = JIT && P.jitter == RTX_JITTER_PHILOX;
            const bool odd = ((kd * n_aa + ka) & 1) != 0;
            f3 jr = jr_odd;
            if (philox && !odd) {
                uint32_t w[4];
                jitter_block(P, cc, j, (kd * n_aa + ka) >> 1, w);
                jr = jitter_rnd(w, 0);
                jr_odd = jitter_rnd(w, 1);
            }
            // (two calls, each with a constant pointer: a selected one keeps jr in scratch)
            const f3 o = philox ? sample_origin<JIT>(P, cc, j, kd, ka, &jr) : sample_origin<JIT>(P, cc, j, kd, ka);
#pragma unroll 1
            for (int kt = 0; kt < n_times; ++kt) {
                const float time = P.times[L.tbase + kt];
                const SceneView S = sample_scene<false>(P.S);
                HHit hh;  // (hierarchy hits only: never filled here)
                const Hit h = closest_hit<MESH, false, false>(S, o, ddir, time, tl, hs, hh, bin, nullptr, -1);
                if (h.obj != -1) {  // (a miss does nothing)
                    ++nhit;
                    const int32_t k = MAT ? resolve_hit<MESH, false>(S, h, hh, o, ddir, time).mat : hit_oid(S, h, false);
                    id_count(t, fill, run, k);
                }
            }
        }
    }
    id_add(t, fill, run.key, run.n);  // the last run
    id_rank(t);
    const int64_t p = (int64_t)rr * ncols + cc;
    const int32_t ranks = L.ranks;
    const bool wide = ((reinterpret_cast<uintptr_t>(L.ids) | reinterpret_cast<uintptr_t>(L.counts)) & 15u) == 0;
    if (L.ids) id_store(L.ids, p, ranks, wide, t.key);
    if (L.counts) id_store(L.counts, p, ranks, wide, t.cnt);
    if (L.other) {
        int32_t written = 0;
#pragma unroll
        for (int r = 0; r < RTX_ID_SLOTS; ++r) written += r < ranks ? t.cnt[r] : 0;
        L.other[p] = nhit - written;
    }
}

// The per-call block of rtx_cast_rays: n caller-built rays as SoA fp32 [3][n] (rtx_intersect's
// layout), the motion times by value, and the output, fp32 [n / group][3].
struct CastLaunch {
    const float* ro;
    const float* rd;
    float* rgb;
    unsigned long long* counters;
    int64_t n;
    int32_t group, n_times;
    float times[RTX_CAST_MAX_TIMES];
};

// scene.py:81-116 for caller-built rays (rtx_cast_rays): one lane traces one sample. Output j
// is the mean of S = group * n_times samples; its sample s is ray j * group + s / n_times at
// times[s % n_times] (time fastest: scene.py:57-69's loop nest for one pixel). The mapping is
// render_block_spp's: the B lanes of a block trace the samples of PPB = B / S consecutive
// outputs, or those of one output in ceil(S / B) rounds; each lane parks its colour in LDS
// and one owner lane per (output, channel) adds the samples in order from +0 and divides
// once -- render_pixel's fp32 sums. S == 1 (PPB = B) stores the lane's own colour: c / 1.0f
// is c; no LDS traffic, no barrier. The parking words are the lane's own words of frame 0
// of its FrameStack ([frame][word][thread]: a lane's column is its own, and its frames are
// dead once its cast_ray has returned), so secondary-ray variants need no LDS beside the
// frames. S is the scene-level view (rtx_scene_create's): no primary bins, shadow bins,
// plane self tests or directional shadow grids -- those hold for the camera's rays only --
// so cast_ray's level-0 self object can skip nothing (occluded reads it only beside
// SceneView::plane_self and DSGrid::self_boxes, both absent: null and dsg_on = 0).
// Every thread reaches every barrier: inactive lanes (ragged last block, lp >= PPB) only
// skip the trace.
template <bool MESH, bool SEC, bool X, bool COUNT>
__global__ RTX_RENDER_BOUNDS(MESH, SEC, X) void k_cast_rays(const SceneView S, const CastLaunch L) {
    constexpr int B = kBlock<X>;
    static_assert(kFrameWords >= 3, "a lane parks its colour in three words of its frame 0");
    __shared__ float lds[SEC ? kFrameLds * kFrameWords * B : 3 * B];
    extern __shared__ float hstack[];  // X: [level][9][thread] (dynamic size)
    const FrameStack fs{lds + threadIdx.x, B};
    const HStack hs{hstack + threadIdx.x, B};
    const int tid = threadIdx.x;
    const int G = L.group, T = L.n_times;
    const int ns = G * T;  // samples per output (the host bounds it by 2^31 - 1)
    const bool single = ns == 1;
    const int PPB = spp_pixels_per_block(ns, B);
    const int rounds = ns <= B ? 1 : (int)(((int64_t)ns + B - 1) / B);
    const float rS = 1.0f / (float)ns;
    const int64_t nout = L.n / G;
    const int64_t out0 = (int64_t)blockIdx.x * PPB;
    Tally tl = {};
    bool any_active = false;
    float acc = 0.0f;  // rounds > 1 (one output per block): lane ch < 3 sums channel ch
    for (int rd = 0; rd < rounds; ++rd) {
        const uint32_t flat = (uint32_t)rd * B + tid;  // the block's sample index
        int lp, s;
        if (ns < B) {
            lp = udiv_small((int)flat, ns, rS, s);
        } else {  // one output per block: its samples in order
            lp = flat < (uint32_t)ns ? 0 : 1;
            s = (int)flat;
        }
        const int64_t j = out0 + lp;
        const bool active = lp < PPB && j < nout;
        f3 c = mk(0.0f, 0.0f, 0.0f);
        if (active) {
            any_active = true;
            const uint32_t g = T == 1 ? (uint32_t)s : (uint32_t)s / (uint32_t)T;
            const int kt = T == 1 ? 0 : (int)((uint32_t)s - g * (uint32_t)T);
            const int64_t i = j * G + g;
            const Ray r = soa_ray(L.ro, L.rd, L.n, i);
            c = cast_ray<MESH, SEC, X, COUNT>(S, r.o, r.d, L.times[kt], tl, fs, hs);
        }
        if (single) {
            if (active) put3(L.rgb, j, c);
            continue;
        }
        lds[tid] = c.x;
        lds[B + tid] = c.y;
        lds[2 * B + tid] = c.z;
        __syncthreads();
        if (rounds == 1) {  // (output, channel) pairs, each summed in order by one lane
            for (int q = tid; q < 3 * PPB; q += B) {
                const int pp = q / 3, ch = q - 3 * pp;
                if (out0 + pp < nout) {
                    const float* src = lds + ch * B + pp * ns;
                    float a = 0.0f;
                    for (int k = 0; k < ns; ++k) a += src[k];
                    L.rgb[3 * (out0 + pp) + ch] = a / (float)ns;
                }
            }
        } else if (tid < 3) {  // this round's samples of the block's output
            const int hi = min(ns - rd * B, B);
            const float* src = lds + tid * B;
            for (int k = 0; k < hi; ++k) acc += src[k];
        }
        __syncthreads();  // the words are frames again in the next round
    }
    if (rounds > 1 && tid < 3 && out0 < nout) L.rgb[3 * out0 + tid] = acc / (float)ns;
    flush_tally<COUNT>(tl, L.counters, any_active);
}

#if !defined(RTX_EXT_TU)  // defined once, in rtx_api.hip
// The heavy tiles' chunks (one wave per chunk, launched as one-wave blocks), before the
// render kernel: items (bin, chunk). A launch of rows (row0, nrows) or 8-row groups
// (gphase + k gstride) runs only the chunks of its tiles. mode (option chunk_mode):
// bit 0 stages each chunk's face records in LDS first (mesh_chunk_lds); bit 1 hands the
// items to the XCDs in runs of 16 consecutive chunks (xcd_block: the dispatcher deals
// blocks round-robin to the 8 XCDs, so neighbouring chunks -- which share faces -- would
// otherwise pull the same records into all eight L2s).
__global__ __launch_bounds__(64) void k_mesh_chunks(const KParams* __restrict__ Pp, const Launch L,
                                                    const int2* __restrict__ items, int32_t n, uint2* __restrict__ out,
                                                    int32_t mode) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ ChunkLds sh;
#endif
    const uint32_t b = (mode & 2) ? xcd_block(blockIdx.x, gridDim.x, 1) : blockIdx.x;
    const int32_t w = __builtin_amdgcn_readfirstlane((int32_t)b);
    if (w >= n) return;
    const int2 it = items[w];
    const int32_t ty = it.x / Pp->S.bins_x;  // the tile's 8-row group
    const bool mine = L.gstride > 0 ? (ty >= L.gphase && (ty - L.gphase) % L.gstride == 0)
                                    : (ty * 8 + 8 > L.row0 && ty * 8 < L.row0 + L.nrows);
    if (!mine) return;
    const int lane = threadIdx.x & 63;
    const int64_t slot = Pp->S.bin_heavy[it.x];
#if defined(__HIP_DEVICE_COMPILE__)
    if (mode & 1) {
        out[(slot + it.y) * 64 + lane] = mesh_chunk_lds(*Pp, it.x, it.y, lane, sh);
        return;
    }
#endif
    out[(slot + it.y) * 64 + lane] = mesh_chunk(*Pp, it.x, it.y, lane);
}
// (v * 255.0) truncated to uint8, four values per thread: one 16-byte load and one 4-byte
// store (fb 16-byte and out 4-byte aligned; rtx_fb_to_rgb8 checks), the tail one by one.
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int)((double)v * 255.0); }
__global__ __launch_bounds__(256) void k_to_rgb8(const float* __restrict__ fb, uint8_t* __restrict__ out, int64_t n) {
    const int64_t i = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(fb + i);
        *reinterpret_cast<uchar4*>(out + i) = make_uchar4(to_u8(v.x), to_u8(v.y), to_u8(v.z), to_u8(v.w));
    } else {
        for (int64_t k = i; k < n; ++k) out[k] = to_u8(fb[k]);
    }
}
// Shadow-grid cells from their objects' rectangles (rtx_api.hip dir_shadow_grids): cell c of
// grid `off` ORs the bits of every rectangle of that grid holding it -- the host loop's
// result, without the host filling (and uploading) 2 MB per light.
__global__ __launch_bounds__(256) void k_dsg_fill(const DSRect* __restrict__ r, int32_t nr, DSCell* __restrict__ cells,
                                                  int64_t ncells, int32_t G) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const int64_t gg = (int64_t)G * G, off = c / gg * gg;
    const int32_t q = (int32_t)(c - off), jy = q / G, ix = q - jy * G;
    DSCell v{0u, 0u};
    // the rectangles come grid by grid (off ascending, dir_shadow_grids): this grid's range
    int32_t lo = 0, hi = nr;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (r[mid].off < off) lo = mid + 1;
        else hi = mid;
    }
    for (int32_t k = lo; k < nr && r[k].off == off; ++k) {
        const DSRect R = r[k];
        if (ix >= R.i0 && ix <= R.i1 && jy >= R.j0 && jy <= R.j1) {
            v.obj |= R.bit;
            v.root |= R.root;
        }
    }
    cells[c] = v;
}

// Fills a camera's direction table (rtx_camera_set, once per upload, after the tables and the
// frame parameters are on the device): one lane per slot, so a wave writes one 8x8 tile's 768
// contiguous bytes. nslots is a whole number of tiles (ray_table_slots).
__global__ __launch_bounds__(256) void k_ray_dirs(const KParams* __restrict__ Pp, float* __restrict__ out, int64_t nslots) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nslots) return;
    const f3 d = ray_table_entry(*Pp, s);
    float* o = out + 3 * s;
    o[0] = d.x;
    o[1] = d.y;
    o[2] = d.z;
}

// Camera uploads (rtx_api.hip pinned_upload): 16-byte words from the scene's pinned host
// buffer, read over the bus by the kernel itself -- no copy engine.
__global__ __launch_bounds__(256) void k_stage_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_to_rgb8_unaligned(const float* __restrict__ fb, uint8_t* __restrict__ out,
                                                           int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = to_u8(fb[i]);
}
#endif
#endif  // !__HIPCC_RTC__

}  // namespace rtx
