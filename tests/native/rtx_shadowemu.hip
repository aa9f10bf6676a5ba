// rtx_shadowemu.hip — TESTS ONLY. The host emulation (rtx_hostemu.hip: the device source of
// librtx.so run on the CPU) plus what the shadow-bin tests need: the table rtx_camera_set
// builds (rtx_api.hip shadow_bins), a check of it against the device's own occlusion test
// at every pixel's level-0 hit point, and a render that reads it.
#include "rtx_hostemu.hip"

namespace {
// The emulated camera of a flat scene (no mesh, no hierarchy).
int flat_cam(EmuCam& F, const rtx_scene_desc* sd, const rtx_camera_desc* cd) {
    if (int rc = F.init(sd, cd)) return rc;
    if (F.H.has_mesh || F.H.has_ext) return fail(RTX_ERR_INVALID, "shadowemu: flat scenes only");
    return RTX_OK;
}
}  // namespace

// The shadow bins of a camera: out[bin * n_lights + light] (margin: shadow_bins' test knob,
// 1 = the product's). Returns the number of words (0: the camera gets none); *ms, if given,
// the host time of the build (best of reps).
extern "C" int64_t rtx_shadowemu_masks(const rtx_scene_desc* sd, const rtx_camera_desc* cd, double margin, uint32_t* out,
                                       int64_t cap, int reps, double* ms) {
    EmuCam F;
    if (flat_cam(F, sd, cd)) return -1;
    if (!F.T.bins) return 0;
    std::vector<uint32_t> m;
    double best = INFINITY;
    for (int r = 0; r < (reps > 0 ? reps : 1); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        if (!shadow_bins(F.H, cd, F.T.bmask, F.T.bins_x, m, margin)) return 0;
        best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    if (ms) *ms = best;
    for (int64_t i = 0; i < (int64_t)m.size() && i < cap; ++i) out[i] = m[i];
    return (int64_t)m.size();
}

// For every pixel's level-0 hit point (the camera ray as render_pixel casts it, every motion
// time), every light and every sphere and box: the object alone, by the device's own
// occluded() of a scene that holds nothing else. res[0]: tests that found the object
// occluding; res[1]: those whose bit in masks[bin * n_lights + light] is clear (the table
// would have skipped a test that passes); res[2]: level-0 hits.
extern "C" int rtx_shadowemu_check(const rtx_scene_desc* sd, const rtx_camera_desc* cd, const uint32_t* masks, int64_t* res) {
    EmuCam F;
    if (int rc = flat_cam(F, sd, cd)) return rc;
    if (!F.T.bins) return fail(RTX_ERR_INVALID, "shadowemu: the camera has no bins");
    const KParams& k = F.k;
    const HostScene& H = F.H;
    const int32_t NL = H.n_lights;
    int64_t occl = 0, bad = 0, hits = 0;
    for (int32_t row = 0; row < k.height; ++row)
        for (int32_t cc = 0; cc < k.ncols; ++cc)
            for (int32_t kt = 0; kt < k.n_times; ++kt) {
                Tally tl = {};
                float hst[kMaxHLevels * 9];
                const HStack hs{hst, 1};
                const int32_t bin = primary_bin(k.S, row & ~7, cc & ~7);
                const int32_t blane = ((row & 7) << 3) | (cc & 7);
                const int j = k.height - 1 - row;
                const float time = k.times[kt];
                const f3 o = sample_origin<false>(k, cc, j, 0, 0);
                const f3 d = normalize(sub(pixel_focal(k, cc, j), ld3(k.dof_o)));
                HHit hh;
                const Hit h = closest_hit<false, false, true>(k.S, o, d, time, tl, hs, hh, bin, nullptr, blane);
                if (h.obj == -1) continue;
                ++hits;
                const Surface sf = resolve_hit<false, false>(k.S, h, hh, o, d, time);
                for (int32_t li = 0; li < NL; ++li) {
                    const DLight& L = H.lights[li];
                    const bool point = L.type == LIGHT_POINT;
                    const f3 sdir = point ? sub(ld3(L.vec), sf.position) : ld3(L.negvec);
                    const double t_max = point ? 1.0 : (double)INFINITY;
                    for (int32_t q = 0; q < H.n_sphere + H.n_box; ++q) {
                        SceneView V{};
                        V.objs = (cptr<DObj>)&H.objs[H.n_plane + q];
                        V.n_objs = 1;
                        const bool sphere = q < H.n_sphere;
                        V.n_sphere = sphere ? 1 : 0;
                        V.n_box = sphere ? 0 : 1;
                        if (!occluded<false, false, true>(V, sf.position, sdir, t_max, time, tl, hs)) continue;
                        ++occl;
                        const int32_t kk = sphere ? q : q - H.n_sphere;
                        const uint32_t bit = 1u << ((sphere ? 0 : 16) + (kk & 15));
                        if (!(masks[(int64_t)bin * NL + li] & bit)) ++bad;
                    }
                }
            }
    res[0] = occl;
    res[1] = bad;
    res[2] = hits;
    return RTX_OK;
}

// (render_block jitters as the camera says, as rtx_hostemu_render does; the pinhole cameras
// that get shadow bins have none.)
// rtx_hostemu_render of a flat scene with the camera's shadow bins bound (use_masks) or not.
// *bound: 1 when the frame read the table.
extern "C" int rtx_shadowemu_render(const rtx_scene_desc* sd, const rtx_camera_desc* cd, int use_masks, float* fb,
                                    uint64_t* counters, int threads, int* bound_out) {
    EmuCam F;
    if (int rc = flat_cam(F, sd, cd)) return rc;
    if (!use_masks) F.k.S.bin_shadow = nullptr;
    uint64_t tot[RTX_COUNTERS] = {};
    render_block(F, 0, F.k.height, fb, tot, threads);
    for (int q = 0; q < RTX_COUNTERS; ++q) counters[q] = tot[q];
    *bound_out = F.k.S.bin_shadow != nullptr;
    return RTX_OK;
}
