// Pooled embedding head of a classification-style ReID backbone (FM_OP_POOLHEAD; models/onnx_graph.py): ONE launch per
// network pass, one workgroup per sample:
//   global average pool over HW (fp32) -> optional per-channel affine (the BN neck folded to scale / shift, fp32)
//   (GeM pooling, a template mode of the kernel in reidhead_kernel.h: the pool sums max(x, eps)^p and the mean takes the
//   p-th root before the neck; instantiated in reidhead_gem.hip -- this file's plain instantiation is the code without it)
//   -> optional FC C -> D (fp16 weights, fp32 bias with any BatchNorm folded in, optional ReLU) -> L2 normalise
//   -> the row to ctx->emb and to its page-locked mirror, where ops.hip head_kernel writes its rows (no export launch
//   behind the network: the emb_host contract of extract.hip).
// ResNet-50's head is C = 2048 over an 8 x 4 map.  head_kernel gives every output row to ONE thread that walks the C
// weights of its row: at C = 2048 that is 4096 dependent steps per thread over addresses 4 KB apart between lanes.  Here
// a WAVEFRONT owns an output row: 64 lanes x 16 bytes = 512 consecutive weights per step (one 1 KB line run), fp32 FMAs
// against the pooled vector in LDS, then a cross-lane sum -- C / 512 steps per row instead of C / 8 -- and it works on 8
// rows at a time, so that 8 independent 16-byte loads per lane are in flight per step.
// LDS: part[max(C, 8 * PH_T)] | pooled[C] | feat[D] (FC only) | red[PH_T / 64] floats: 48 KB at C = D = 4096, the limit.
#include "reidhead_kernel.h"


// (reidhead_gem.hip; arguments checked here)
void launch_poolhead_gem(const f16* in, int in_cs, int in_coff, int N, int HW, int C, int D, const float* scale, const float* shift,
                         const f16* w, const float* b, int relu, float* out, float* mirror, hipStream_t s, float gem_p, float gem_eps,
                         size_t shmem);

size_t poolhead_lds_bytes(int C, int D, bool fc) {
    const int c8n = C / 8;
    const int groups = c8n < PH_T ? PH_T / c8n : 1;
    return sizeof(float) * ((size_t)groups * C + C + (fc ? D : 0) + PH_T / 64);
}

// scale / shift: both or neither; w == nullptr: no FC (then D == C); gem_p > 0: GeM pooling with that exponent and clamp gem_eps
int launch_poolhead(const f16* in, int in_cs, int in_coff, int N, int HW, int C, int D, const float* scale, const float* shift,
                    const f16* w, const float* b, int relu, float* out, float* mirror, hipStream_t s, float gem_p, float gem_eps) {
    FM_CHECK_ARG(in && out && N >= 1 && HW >= 1 && C >= 8 && C % 8 == 0 && C <= PH_MAX && D >= 1 && D <= PH_MAX);
    FM_CHECK_ARG(in_cs % 8 == 0 && in_coff % 8 == 0 && in_coff + C <= in_cs && (scale == nullptr) == (shift == nullptr));
    FM_CHECK_ARG(w ? b != nullptr : D == C);
    const size_t shmem = poolhead_lds_bytes(C, D, w != nullptr);
    FM_CHECK_ARG(shmem <= PH_LDS_MAX);
    if (gem_p > 0.f) {
        FM_CHECK_ARG(gem_p >= 0.5f && gem_p <= 16.f && gem_eps > 0.f && gem_eps <= 1.f);
        launch_poolhead_gem(in, in_cs, in_coff, N, HW, C, D, scale, shift, w, b, relu, out, mirror, s, gem_p, gem_eps, shmem);
    } else {
        hipLaunchKernelGGL(poolhead_kernel<GEM_NONE>, dim3(N), dim3(PH_T), shmem, s, in, in_cs, in_coff, HW, C, D, scale, shift, w,
                           b, relu, out, mirror, 0.f, 0.f);
    }
    FM_HIP(hipGetLastError());
    return 0;
}
