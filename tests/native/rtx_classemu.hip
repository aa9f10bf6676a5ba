// rtx_classemu.hip — TESTS ONLY. The host emulation (rtx_hostemu.hip: the device source of
// librtx.so run on the CPU) plus what the tile-class tests need: the class records
// rtx_camera_set builds (rtx_api.hip sb_bin / tile_classes), with the test knobs of their
// margins, and a check of every flag at every pixel against the device's own hit and
// occlusion tests. The renders are rtx_hostemu_render / rtx_hostemu_render_rows of this
// library (option tile_class of this library's copy of the options).
#include "rtx_hostemu.hip"

// The class records of a camera: out[2 * bin] = the bin's object mask, out[2 * bin + 1] = its
// class word. margin: shadow_bins' test knob (1 = the product's; 0: no 2-pixel pad, no growth);
// cls_rho: 0 = the plane_self bound without its growth by rho. Returns the number of bins
// (0: the camera gets no records), -1 on an error.
extern "C" int64_t rtx_classemu_records(const rtx_scene_desc* sd, const rtx_camera_desc* cd, double margin, double cls_rho,
                                        uint32_t* out, int64_t cap) {
    EmuCam F;
    if (F.init(sd, cd, false)) return -1;
    if (!F.T.tclass) return 0;
    SbScene S;
    if (!shadow_bins_scene(F.H, cd, F.T.bins_x, margin, S)) return 0;
    S.cls_rho = cls_rho;
    const int64_t nbin = (int64_t)S.bins_x * S.bins_y;
    std::vector<uint2> rec((size_t)nbin);
    tile_classes(S, cd->xs, cd->ys, F.T.bmask.data(), F.T.pself ? F.T.pself_lim.data() : nullptr, rec.data());
    for (int64_t b = 0; b < nbin && 2 * b + 1 < cap; ++b) {
        out[2 * b] = rec[(size_t)b].x;
        out[2 * b + 1] = rec[(size_t)b].y;
    }
    return nbin;
}

// The records the camera's own table holds (what a render reads), same layout.
extern "C" int64_t rtx_classemu_bound(const rtx_scene_desc* sd, const rtx_camera_desc* cd, uint32_t* out, int64_t cap) {
    EmuCam F;
    if (F.init(sd, cd, false)) return -1;
    if (F.k.S.bin_class == nullptr) return 0;
    const int64_t nbin = (int64_t)F.T.sbs.bins_x * F.T.sbs.bins_y;
    for (int64_t b = 0; b < nbin && 2 * b + 1 < cap; ++b) {
        out[2 * b] = F.k.S.bin_class[b].x;
        out[2 * b + 1] = F.k.S.bin_class[b].y;
    }
    return nbin;
}

// Every flag of rec (rtx_classemu_records' layout) at every pixel of its bin, by the device's
// own tests on the pixel's camera ray with nothing culled (no bins, no tables):
//   SKY         closest_hit misses;
//   PLANE       closest_hit's hit is object 0;
//   UNSHADOWED  from that hit's point, occluded() of the whole scene (the plane included, no
//               self-test skip, no shadow bins) is false for every light.
// res: {SKY pixels, of them hits; PLANE pixels, of them not on object 0; UNSHADOWED (pixel,
// light) tests, of them occluded}.
extern "C" int rtx_classemu_check(const rtx_scene_desc* sd, const rtx_camera_desc* cd, const uint32_t* rec, int64_t* res) {
    EmuCam F;
    if (int rc = F.init(sd, cd, false)) return rc;
    if (F.H.has_mesh || F.H.has_ext) return fail(RTX_ERR_INVALID, "classemu: flat scenes only");
    if (!F.T.bins) return fail(RTX_ERR_INVALID, "classemu: the camera has no bins");
    const KParams& k = F.k;
    const HostScene& H = F.H;
    SceneView V = k.S;  // nothing culled, nothing skipped
    V.bins_on = 0;
    V.plane_self = nullptr;
    V.bin_shadow = nullptr;
    V.bin_class = nullptr;
    V.dsg_on = 0;
    for (int q = 0; q < 6; ++q) res[q] = 0;
    for (int32_t row = 0; row < k.height; ++row)
        for (int32_t cc = 0; cc < k.ncols; ++cc)
            for (int32_t kt = 0; kt < k.n_times; ++kt) {
                const int32_t bin = primary_bin(k.S, row & ~7, cc & ~7);
                const uint32_t cls = rec[2 * (int64_t)bin + 1];
                if (cls == 0u) continue;
                Tally tl = {};
                float hst[kMaxHLevels * 9];
                const HStack hs{hst, 1};
                const int j = k.height - 1 - row;
                const float time = k.times[kt];
                const f3 o = sample_origin<false>(k, cc, j, 0, 0);
                const f3 d = primary_dir(k, cc, j, 0);
                HHit hh;
                const Hit h = closest_hit<false, false, true>(V, o, d, time, tl, hs, hh);
                if (cls & kTileSky) {
                    ++res[0];
                    if (h.obj != -1) ++res[1];
                }
                if (cls & kTilePlane) {
                    ++res[2];
                    if (h.obj != 0) ++res[3];
                }
                if ((cls & kTileUnshadowed) && h.obj != -1) {
                    const Surface sf = resolve_hit<false, false>(V, h, hh, o, d, time);
                    for (int32_t li = 0; li < H.n_lights; ++li) {
                        const DLight& L = H.lights[li];
                        const bool point = L.type == LIGHT_POINT;
                        const f3 sdir = point ? sub(ld3(L.vec), sf.position) : ld3(L.negvec);
                        const double t_max = point ? 1.0 : (double)INFINITY;
                        ++res[4];
                        if (occluded<false, false, true>(V, sf.position, sdir, t_max, time, tl, hs)) ++res[5];
                    }
                }
            }
    return RTX_OK;
}
