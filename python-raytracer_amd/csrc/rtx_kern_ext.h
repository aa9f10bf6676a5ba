// The launchers of the hierarchy/texture kernels (rtx_launch.h), written once for both values
// of MESH: rtx_kern_ext_m0.hip and rtx_kern_ext_m1.hip include this and define the exported
// names for theirs, so the two halves still compile in parallel.
#pragma once

#include <hip/hip_runtime.h>

#define RTX_EXT_TU 1
#include "rtx_kernels.h"
#include "rtx_split.h"
#include "rtx_launch.h"

namespace rtx {

template <bool MESH>
hipError_t launch_render_ext(int sel, const RenderLaunch& r, const Launch& L) {
    const dim3 g(r.nblocks, r.nframes), b(kBlock<true>);
    with_bools([&](auto S, auto C, auto J) {
        if (r.spp) hipLaunchKernelGGL((k_render_spp<MESH, S(), true, C(), J()>), g, b, r.lds_bytes, r.stream, r.kp, L);
        else hipLaunchKernelGGL((k_render<MESH, S(), true, C(), J()>), g, b, r.lds_bytes, r.stream, r.kp, L);
    }, (sel & 8) != 0, (sel & 2) != 0, (sel & 1) != 0);
    return hipGetLastError();
}

template <bool MESH>
hipError_t launch_split(int sel, int pass, const RenderLaunch& r, const Launch& L, const SplitBuf& sb) {
    const bool sec = (sel & 8) != 0, cnt = (sel & 2) != 0, jit = (sel & 1) != 0;
    const dim3 g(r.nblocks), b(kBlock<true>);
    if (pass == 0)
        with_bools([&](auto S, auto C, auto J) {
            hipLaunchKernelGGL((k_split_trace<MESH, S(), C(), J()>), g, b, r.lds_bytes, r.stream, r.kp, L, sb);
        }, sec, cnt, jit);
    else if (pass == 1)
        with_bools([&](auto C) {
            hipLaunchKernelGGL((k_split_shadow<MESH, C()>), g, b, r.lds_bytes, r.stream, r.kp, L, sb);
        }, cnt);
    else
        with_bools([&](auto S) { hipLaunchKernelGGL((k_split_shade<MESH, S()>), g, b, 0, r.stream, r.kp, L, sb); }, sec);
    return hipGetLastError();
}

template <bool MESH>
hipError_t launch_cast_ext(int sel, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const SceneView& S,
                           const CastLaunch& L) {
    with_bools([&](auto SEC, auto C) {
        hipLaunchKernelGGL((k_cast_rays<MESH, SEC(), true, C()>), dim3(nblocks), dim3(kBlock<true>), lds_bytes, stream,
                           S, L);
    }, (sel & 8) != 0, (sel & 2) != 0);
    return hipGetLastError();
}

template <bool MESH>
hipError_t launch_occlusion_ext(bool jitter, unsigned nblocks, size_t lds_bytes, hipStream_t stream, const KParams* kp,
                                const OccLaunch& L) {
    with_bools([&](auto J) {
        hipLaunchKernelGGL((k_occlusion<MESH, true, J()>), dim3(nblocks), dim3(kBlock<true>), lds_bytes, stream, kp, L);
    }, jitter);
    return hipGetLastError();
}

}  // namespace rtx
