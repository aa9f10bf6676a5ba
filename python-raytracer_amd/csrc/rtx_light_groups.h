// rtx_light_groups.h — the light-group pass of librtx.so (rtx_render_light_groups, DESIGN.md
// 6aj): one trace of every sample's ray chain, one shadow test per light and level, and one
// colour per light group. Included by rtx_api.hip only: the render kernels and the sources
// handed to hiprtc (rtx_trace.h, rtx_kernels.h) do not see it, so they compile as before.
//
// Why plane g is rtx_render's image of the scene edited to hold only group g's lights (in
// their order) and the ambient term only where ambient_group == g:
//  * no ray of this renderer depends on a light: closest hits, reflect / refract children and
//    shadow rays are functions of the geometry, so the chain and every light's `occluded`
//    answer are the edited scene's (the per-light tables occluded reads -- shadow bins, plane
//    self tests, light and shadow grids -- are indexed by the light and only skip tests that
//    cannot pass);
//  * regular_lighting starts `colour` at +0 and performs one `add` per unoccluded light in
//    light order, so not adding a light is its absence;
//  * a zero ambient adds mul(0, diffuse) = +-0 to a sum that is never -0 (it starts at +0, and
//    x + y is -0 only when both are), which leaves it unchanged: the other groups skip the add;
//  * the per-level clamp, the sample sum from +0 and the one division are applied per group
//    exactly as cast_ray and render_pixel apply them to the one colour.
#pragma once

#include "rtx_kernels.h"

namespace rtx {

// The per-call block: rows [row0, row0 + nrows) of the strip, the window of motion times
// P.times[tbase .. tbase + n_times), the planes ([n_groups][nrows][ncols][3], `plane` floats
// each) and the light table by value: light li's group is nibble li of grp (15: none, its
// shadow ray is not traced), `used` has bit li set for every light in a group.
struct LightGroupsLaunch {
    float* out;
    int64_t plane;
    int32_t row0, nrows, tbase, n_groups;
    int32_t ambient_group;
    uint32_t used;
    uint64_t grp_lo, grp_hi;  // lights 0-15, 16-31
};

// A chain level as the unwinding needs it, independent of the lights' grouping: the ray's
// direction, the hit position, the shading normal (negated inside a refraction), the material
// (bit 31: the level ends the chain) and the lights whose shadow ray is free.
struct LgRec {
    f3 dir, pos, n;
    uint32_t mat, free;
};
constexpr int kLgWords = 11;
constexpr uint32_t kLgEnd = 0x80000000u;
// Levels kept in LDS, [level][word][thread]; deeper levels of a chain (rare) go to a per-lane
// private array. 4 levels of 11 words are 44 KB per 256-thread block: 3 blocks (12 waves) share
// a CU's 160 KB, which is what the kernels' VGPR allocation allows anyway.
constexpr int kLgLds = 4;
struct LgStack {
    float* base;  // the thread's word 0 of level 0
    int stride;
    __device__ __forceinline__ void put(int k, const LgRec& r) const {
        float* p = base + k * kLgWords * stride;
        p[0] = r.dir.x; p[stride] = r.dir.y; p[2 * stride] = r.dir.z;
        p[3 * stride] = r.pos.x; p[4 * stride] = r.pos.y; p[5 * stride] = r.pos.z;
        p[6 * stride] = r.n.x; p[7 * stride] = r.n.y; p[8 * stride] = r.n.z;
        p[9 * stride] = __builtin_bit_cast(float, r.mat);
        p[10 * stride] = __builtin_bit_cast(float, r.free);
    }
    __device__ __forceinline__ LgRec get(int k) const {
        const float* p = base + k * kLgWords * stride;
        LgRec r;
        r.dir = f3{p[0], p[stride], p[2 * stride]};
        r.pos = f3{p[3 * stride], p[4 * stride], p[5 * stride]};
        r.n = f3{p[6 * stride], p[7 * stride], p[8 * stride]};
        r.mat = __builtin_bit_cast(uint32_t, p[9 * stride]);
        r.free = __builtin_bit_cast(uint32_t, p[10 * stride]);
        return r;
    }
};

__device__ __forceinline__ int32_t lg_group(const LightGroupsLaunch& L, int li) {
    const uint64_t w = li < 16 ? L.grp_lo : L.grp_hi;
    return (int32_t)((w >> ((li & 15) * 4)) & 15u);
}

// regular_lighting's shadow tests at a hit (scene.py:150-167), one `occluded` per grouped
// light with the arguments regular_lighting gives it at that level: bit li = light li's shadow
// ray is free. Lights in no group are not tested.
template <bool MESH>
__device__ __forceinline__ uint32_t lg_free_lights(const SceneView& S, f3 pos, float time, Tally& tl, const HStack& hs,
                                                  int32_t self_obj, int32_t sbin, uint32_t used) {
    cptr<uint32_t> sbm = nullptr;
#if RTX_SHADOW_BINS
    if (sbin >= 0 && S.bin_shadow != nullptr)  // (wave-uniform)
        sbm = S.bin_shadow + (int64_t)wave_uniform(sbin) * RTX_NLIGHTS(S);
#endif
    uint32_t free = 0u;
    for (int li = 0; li < RTX_NLIGHTS(S); ++li) {
        if (!((used >> li) & 1u)) continue;
        const DLight L = S.lights[li];
        f3 sdir;
        double t_max;
        if (L.type == LIGHT_POINT) {
            sdir = sub(ld3(L.vec), pos);
            t_max = 1.0;
        } else {
            sdir = ld3(L.negvec);
            t_max = INFINITY;
        }
        if (!occluded<MESH, false, false>(S, pos, sdir, t_max, time, tl, hs, nullptr, li, self_obj, sbm ? sbm[li] : ~0u))
            free |= 1u << li;
    }
    return free;
}

// regular_lighting's colour of a recorded level (scene.py:168-187), per group: each free
// light's term computed once with regular_lighting's operations and added to its group's sum
// in light order, the ambient term added to the ambient group's only.
template <int G>
__device__ __forceinline__ void lg_shade(const SceneView& S, const LgRec& r, const DMat& m, const LightGroupsLaunch& L,
                                         f3 (&colour)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) colour[g] = mk(0.0f, 0.0f, 0.0f);
    const f3 diffuse = ld3(m.diffuse);
    for (int li = 0; li < RTX_NLIGHTS(S); ++li) {
        const bool lit = ((r.free >> li) & 1u) != 0u;
        if (!RTX_ANY(lit)) continue;
        const int32_t grp = lg_group(L, li);  // (wave-uniform)
        if (lit) {
            const DLight Lt = S.lights[li];
            const bool point = Lt.type == LIGHT_POINT;
            const f3 light_dir = point ? normalize(sub(ld3(Lt.vec), r.pos)) : ld3(Lt.ndir);
            const f3 lambert = scale(diffuse, pos_part(dot(r.n, light_dir)));
            f3 ls = lambert;
            if (!m.spec_zero) {
                const f3 half_vect = normalize(sub(light_dir, r.dir));
                const float nh = dot(r.n, half_vect);
                const double base = nh > 0.0f ? (double)nh : 0.0;
                const f3 specular = scale(ld3(m.specular), (float)spec_pow(base, m, S.pow_bits));
                ls = add(lambert, specular);
            }
            const f3 term = mul(ld3(Lt.cp), ls);
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (grp == g) colour[g] = add(colour[g], term);
        }
    }
    const f3 amb = mul(ld3(S.ambient), diffuse);
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (L.ambient_group == g) colour[g] = add(colour[g], amb);
}

// cast_ray (scene.py:81-116) with one colour per light group: the chain is traced once, going
// down each level leaves an LgRec (the SEC kernels; a kernel of primary and shadow rays shades
// its one level at once), coming back up each level is shaded per group and folded into the
// groups' tails with cast_ray's per-level clamp. Misses, total internal reflection and the
// depth limit behave as in cast_ray: the tails start black.
template <bool MESH, bool SEC, int G>
__device__ __forceinline__ void cast_ray_groups(const SceneView& S, f3 o, f3 d, float time, Tally& tl, const LgStack& st,
                                                const HStack& hs, int32_t bin, const LightGroupsLaunch& L, f3 (&tail)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) tail[g] = mk(0.0f, 0.0f, 0.0f);
    int nfr = 0;
    LgRec deep[SEC ? kMaxDepth - kLgLds : 1];  // levels kLgLds.. (private)
    bool in_shape = false;
    for (int level = 0; level < (SEC ? kMaxDepth : 1); ++level) {
        HHit hh;  // (hierarchy hits only: never filled here)
        const Hit h = closest_hit<MESH, false, false>(S, o, d, time, tl, hs, hh, level == 0 ? bin : -1, nullptr, -1);
        if (h.obj == -1) break;  // miss -> black
        const Surface sf = resolve_hit<MESH, false>(S, h, hh, o, d, time);
        const DMat m = RTX_MAT(S, sf.mat);
        f3 n = sf.normal;
        bool chain = false, tir = false;
        f3 next_o = o, next_d = d;
        if (SEC && m.type == MAT_MIRROR) {  // reflect; child with in_shape = False
            const f3 rdir = reflect(d, n);
            next_o = add(sf.position, scale(rdir, 0.01f));
            next_d = rdir;
            chain = true;
        } else if (SEC && m.type == MAT_REFRACTIVE) {  // the negated normal also shades
            const float eta = in_shape ? m.eta_in : m.eta_out;
            if (in_shape) n = neg(n);
            const f3 rdir = refract(d, n, eta);
            tir = is_zero(rdir);  // total internal reflection -> black child
            next_o = add(sf.position, scale(rdir, 0.0001f));
            next_d = rdir;
            chain = true;
        }
        // a camera ray's hit (level 0) tells occluded which flat object it lies on
        LgRec r;
        r.dir = d;
        r.pos = sf.position;
        r.n = n;
        r.mat = (uint32_t)sf.mat | (chain ? 0u : kLgEnd);
        r.free = lg_free_lights<MESH>(S, sf.position, time, tl, hs, level == 0 ? h.obj : -1, level == 0 ? bin : -1, L.used);
        if (!SEC) {
            f3 c[G];
            lg_shade<G>(S, r, m, L, c);
#pragma unroll
            for (int g = 0; g < G; ++g) tail[g] = clamp01(c[g]);
            break;
        }
        if (nfr < kLgLds)
            st.put(nfr, r);
        else
            deep[nfr - kLgLds] = r;
        ++nfr;
        if (!chain || tir) break;
        in_shape = m.type == MAT_REFRACTIVE ? !in_shape : false;
        o = next_o;
        d = next_d;
    }
    if (SEC) {
        for (int k = nfr - 1; k >= 0; --k) {
            LgRec r;
            if (k < kLgLds)
                r = st.get(k);
            else
                r = deep[k - kLgLds];
            const bool end = (r.mat & kLgEnd) != 0u;
            const DMat m = RTX_MAT(S, (int32_t)(r.mat & ~kLgEnd));
            f3 c[G];
            lg_shade<G>(S, r, m, L, c);
#pragma unroll
            for (int g = 0; g < G; ++g)
                tail[g] = end ? clamp01(c[g]) : clamp01(add(scale(c[g], m.tint), scale(tail[g], m.omt)));
        }
    }
}

// Each light group's colour of a pixel: render_pixel's sample loops (k_resolved's copy of
// them: the same rays, jitter draws and order, time fastest) with cast_ray_groups where
// render_pixel calls cast_ray, G sums from +0 where it has one, and its one division per
// channel. The mapping is k_resolved's: one lane per pixel, an 8x8 tile per wave, the tile's
// primary bin, no pixel-in-tile (a heavy mesh tile walks its face list). G is the number of
// accumulators compiled in (4 or 8); planes g >= n_groups are neither lit nor stored. The sums
// and tails stay in registers; each plane is stored once per pixel. A flat-scene kernel.
template <bool MESH, bool SEC, bool JIT, int G>
__global__ __launch_bounds__(kBlock<false>) void k_light_groups(const KParams* __restrict__ Pp, const LightGroupsLaunch L) {
    constexpr int B = kBlock<false>;
    __shared__ float lg_lds[SEC ? kLgLds * kLgWords * B : 1];
    const LgStack st{lg_lds + threadIdx.x, B};
    const HStack hs{nullptr, B};  // (flat scenes: closest_hit never touches it)
    const KParams& P = *Pp;
    const int32_t ncols = P.ncols;
    Tally tl = {};
    const FirstHit f = first_pixel<false>(P, L.nrows);
    if (!f.in) return;
    const int32_t rr = f.px.r, cc = f.px.c;
    const int32_t bin = RTX_TILE == 1 ? primary_bin(P.S, L.row0 + (rr & ~7), cc & ~7) : -1;
    const int j = P.height - 1 - (L.row0 + rr);  // reference row index (y grows upward)
    f3 colour[G];
#pragma unroll
    for (int g = 0; g < G; ++g) colour[g] = mk(0.0f, 0.0f, 0.0f);
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
                f3 tail[G];
                cast_ray_groups<MESH, SEC, G>(sample_scene<false>(P.S), o, ddir, P.times[L.tbase + kt], tl, st, hs, bin, L,
                                              tail);
#pragma unroll
                for (int g = 0; g < G; ++g) colour[g] = add(colour[g], tail[g]);
            }
        }
    }
    const int64_t p = (int64_t)rr * ncols + cc;
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (g < L.n_groups)
            put3(L.out + g * L.plane, p,
                 mk(sample_mean(P, colour[g].x), sample_mean(P, colour[g].y), sample_mean(P, colour[g].z)));
}

}  // namespace rtx
