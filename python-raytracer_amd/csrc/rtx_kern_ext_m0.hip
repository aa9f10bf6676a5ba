// Hierarchy/texture render kernels with MESH = false (tile and sample-parallel mappings):
// a translation unit of their own so they compile in parallel with the rest of librtx.so.
#include "rtx_kern_ext.h"

namespace rtx {
hipError_t launch_render_ext_m0(int sel, const RenderLaunch& r, const Launch& L) {
    return launch_render_ext<false>(sel, r, L);
}
hipError_t launch_split_m0(int sel, int pass, const RenderLaunch& r, const Launch& L, const SplitBuf& sb) {
    return launch_split<false>(sel, pass, r, L, sb);
}
hipError_t launch_cast_ext_m0(int sel, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const SceneView& S,
                              const CastLaunch& L) {
    return launch_cast_ext<false>(sel, nblocks, lds_bytes, stream, S, L);
}
hipError_t launch_occlusion_ext_m0(bool jitter, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const KParams* kp,
                                   const OccLaunch& L) {
    return launch_occlusion_ext<false>(jitter, nblocks, lds_bytes, stream, kp, L);
}
}  // namespace rtx
