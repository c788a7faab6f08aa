// The GeM instantiations of the pooled embedding head (reidhead_kernel.h; launched through launch_poolhead in reidhead.hip):
// mean(max(x, eps)^p)^(1/p) in place of the average pool -- p == 3 as two multiplies and cbrtf, any other p as powf.
// Built with -fno-slp-vectorize (build.py FILE_FLAGS): see reidhead_kernel.h.
#include "reidhead_kernel.h"

void launch_poolhead_gem(const f16* in, int in_cs, int in_coff, int N, int HW, int C, int D, const float* scale, const float* shift,
                         const f16* w, const float* b, int relu, float* out, float* mirror, hipStream_t s, float gem_p, float gem_eps,
                         size_t shmem) {
    if (gem_p == 3.f)
        hipLaunchKernelGGL(poolhead_kernel<GEM_CUBE>, dim3(N), dim3(PH_T), shmem, s, in, in_cs, in_coff, HW, C, D, scale, shift, w, b,
                           relu, out, mirror, gem_p, gem_eps);
    else
        hipLaunchKernelGGL(poolhead_kernel<GEM_POW>, dim3(N), dim3(PH_T), shmem, s, in, in_cs, in_coff, HW, C, D, scale, shift, w, b,
                           relu, out, mirror, gem_p, gem_eps);
}
