// rtx_launch.h — launchers of the precompiled hierarchy/texture (X) render kernels, which
// live in their own translation units (rtx_kern_ext_m0.hip / _m1.hip, by MESH) so the
// library's largest kernels compile in parallel.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace rtx {
// with_bools(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...): the
// run-time flags of a launch as the template arguments of its kernel variant (every launcher).
template <class F>
void with_bools(F&& f) {
    f();
}
template <class F, class... Bs>
void with_bools(F&& f, bool b, Bs... rest) {
    if (b) with_bools([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_bools([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

struct KParams;
struct Launch;

struct RenderLaunch {
    const KParams* kp;
    unsigned nblocks;
    unsigned nframes;  // gridDim.y: frames of a batched launch (rtx_render_frames)
    size_t lds_bytes;  // dynamic LDS (hierarchy stacks)
    hipStream_t stream;
    bool spp;          // sample-parallel mapping (render_body_spp)
};

// sel: (SEC ? 8 : 0) | (COUNT ? 2 : 0) | (JITTER ? 1 : 0); returns hipGetLastError().
hipError_t launch_render_ext_m0(int sel, const RenderLaunch& r, const Launch& L);
hipError_t launch_render_ext_m1(int sel, const RenderLaunch& r, const Launch& L);

// The split passes of rtx_split.h (pass 0 trace, 1 shadow, 2 shade) with r.nblocks blocks.
struct SplitBuf;
hipError_t launch_split_m0(int sel, int pass, const RenderLaunch& r, const Launch& L, const SplitBuf& sb);
hipError_t launch_split_m1(int sel, int pass, const RenderLaunch& r, const Launch& L, const SplitBuf& sb);

// k_cast_rays (rtx_cast_rays) of the hierarchy/texture variants: nblocks one-wave blocks with
// lds_bytes of dynamic LDS. sel: (SEC ? 8 : 0) | (COUNT ? 2 : 0).
struct SceneView;
struct CastLaunch;
hipError_t launch_cast_ext_m0(int sel, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const SceneView& S,
                              const CastLaunch& L);
hipError_t launch_cast_ext_m1(int sel, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const SceneView& S,
                              const CastLaunch& L);

// k_occlusion (rtx_render_occlusion) of the hierarchy/texture variants: nblocks one-wave blocks
// with lds_bytes of dynamic LDS; jitter: the camera's JITTER variant.
struct OccLaunch;
hipError_t launch_occlusion_ext_m0(bool jitter, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const KParams* kp,
                                   const OccLaunch& L);
hipError_t launch_occlusion_ext_m1(bool jitter, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const KParams* kp,
                                   const OccLaunch& L);
}  // namespace rtx
