// rtx_hostemu_rays.hip — TESTS ONLY. The host emulation (rtx_hostemu.hip, unchanged) with two
// more entry points for tests/test_ray_table.py: the primary-ray direction table a camera gets
// (rtx_api.hip CamTables::rays, filled by the host loop over ray_table_entry) and primary_dir
// evaluated pixel by pixel.
#include "rtx_hostemu.hip"

// The camera's direction table in its own layout (rtx_kernels.h ray_slot), three floats per
// slot, at most cap slots into out. Returns the table's slots; 0: the camera has no table;
// -1: bad input.
extern "C" int64_t rtx_hostemu_ray_table(const rtx_scene_desc* sd, const rtx_camera_desc* cd, float* out, int64_t cap) {
    EmuCam E;
    if (E.init(sd, cd, false)) return -1;
    if (E.k.ray_dirs == nullptr) return 0;
    const int64_t n = ray_table_slots(E.k.height, E.k.ncols);
    if (out) memcpy(out, E.k.ray_dirs, sizeof(float) * 3 * (size_t)std::min(n, cap));
    return n;
}

// primary_dir of every pixel of the strip: out[(r * ncols + cc) * 3 ..], image row r (0 = top).
extern "C" int rtx_hostemu_primary_dirs(const rtx_scene_desc* sd, const rtx_camera_desc* cd, float* out) {
    EmuCam E;
    if (int rc = E.init(sd, cd, false)) return rc;
    const KParams& k = E.k;
    for (int32_t r = 0; r < k.height; ++r)
        for (int32_t cc = 0; cc < k.ncols; ++cc) {
            const f3 d = primary_dir(k, cc, k.height - 1 - r);
            float* o = out + ((size_t)r * k.ncols + cc) * 3;
            o[0] = d.x; o[1] = d.y; o[2] = d.z;
        }
    return RTX_OK;
}
