// Exponential moving average of the flat trainable bucket: ema <- d ema + w p, with d and w = 1 - d formed on the host.  Compiled with the default
// flags, like optim.hip and optim_groups.hip.
//   ema_update_kernel   the stand-alone update: one read of p, one read and one write of ema
//   adamw_ema_kernel    adamw_grouped_kernel's arithmetic (same clip prologue, same segment table) with the update applied to the just-stepped
//                       parameter while it is still in registers: one f32 stream in and one out on top of the step, p is not read again
// The update is written with the round-to-nearest intrinsics, so it is two roundings per element (w p, then the fused multiply-add) whatever the
// contraction flags: d = 0 gives ema == p and d = 1 (w = 0) leaves ema alone, bit for bit, for finite inputs.
#include "optim_common.h"

__device__ __forceinline__ float ema_next(float ema, float p, float d, float w) { return __fmaf_rn(d, ema, __fmul_rn(w, p)); }

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n, float d, float w) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        const float4 ev = *(const float4*)(ema + i), pv = *(const float4*)(p + i);
        *(float4*)(ema + i) = make_float4(ema_next(ev.x, pv.x, d, w), ema_next(ev.y, pv.y, d, w), ema_next(ev.z, pv.z, d, w), ema_next(ev.w, pv.w, d, w));
    }
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, bf16_t* __restrict__ p_bf16, int64_t n, float b1, float b2,
                                                        float eps, float bc1, float bc2_sqrt, float grad_scale, float max_norm,
                                                        const double* __restrict__ partials, int npart, float* __restrict__ norm_out,
                                                        const SegTable tab, int nseg, float* __restrict__ ema, float d, float w) {
    float coef = 1.f;
    if (max_norm > 0.f) {           // (a kernel argument: uniform, the barrier inside is reached by every thread)
        __shared__ double wsum[4];
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < SUMSQ_PER_THREAD; k++) {
            const int idx = threadIdx.x * SUMSQ_PER_THREAD + k;
            if (idx < npart) a += partials[idx];
        }
        const double norm = sqrt(block_sum_f64(a, wsum)) * fabs((double)grad_scale);       // L2 norm of the SCALED gradient
        const double c = (double)max_norm / (norm + 1e-6);                                  // clip_grad_norm_'s coefficient
        coef = c < 1.0 ? (float)c : 1.f;
        if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)norm;
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    int s = 0;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        while (s < nseg - 1 && i >= tab.end[s]) s++;        // i only grows; every tensor starts 8-element aligned, so no float4 straddles a segment
        const float lr = tab.lr[s], wd = tab.wd[s];
        float4 pv = *(const float4*)(p + i), gv = *(const float4*)(g + i), mv = *(const float4*)(m + i), vv = *(const float4*)(v + i);
        const float4 ev = *(const float4*)(ema + i);
        float pa[4] = {pv.x, pv.y, pv.z, pv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
        float ea[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float gg = ga[e] * grad_scale * coef;     // adamw_grouped_kernel's expression sequence, token for token: its bits
            pa[e] *= (1.f - lr * wd);                       // decoupled weight decay
            ma[e] = b1 * ma[e] + (1.f - b1) * gg;
            va[e] = b2 * va[e] + (1.f - b2) * gg * gg;
            const float denom = sqrtf(va[e]) / bc2_sqrt + eps;
            pa[e] -= (lr / bc1) * (ma[e] / denom);
            ea[e] = ema_next(ea[e], pa[e], d, w);           // the average follows the parameter this step leaves behind
        }
        *(float4*)(p + i) = make_float4(pa[0], pa[1], pa[2], pa[3]);
        *(float4*)(m + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
        *(float4*)(v + i) = make_float4(va[0], va[1], va[2], va[3]);
        *(float4*)(ema + i) = make_float4(ea[0], ea[1], ea[2], ea[3]);
        if (p_bf16) {
            uint2 o; o.x = pack_bf2(pa[0], pa[1]); o.y = pack_bf2(pa[2], pa[3]);
            *(uint2*)(p_bf16 + i) = o;
        }
    }
}

static inline unsigned step_blocks(int64_t n) {
    const int64_t blocks = (n / 4 + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

OWL_API int owl_ema_update(void* stream, float* ema, const float* p, int64_t n, float d, float w) {
    OWL_CHECK_ARG(ema && p, "owl_ema_update: null pointer (ema, p)");
    OWL_CHECK_ARG(n > 0 && n % 4 == 0, "owl_ema_update: n must be positive and n %% 4 == 0");
    hipLaunchKernelGGL(ema_update_kernel, dim3(step_blocks(n)), dim3(256), 0, (hipStream_t)stream, ema, p, n, d, w);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_adamw_step_ema(void* stream, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int64_t step, float grad_scale, const int64_t* seg_end,
                               const float* seg_lr, const float* seg_wd, int nseg, float max_norm, const void* workspace, float* norm_out,
                               float* ema, float d, float w) {
    OWL_CHECK_ARG(p && g && m && v && ema, "owl_adamw_step_ema: null pointer (p, g, m, v, ema)");
    OWL_CHECK_ARG(n > 0 && n % 4 == 0, "owl_adamw_step_ema: n must be positive and n %% 4 == 0");
    OWL_CHECK_ARG(step >= 1, "owl_adamw_step_ema: step >= 1");
    SegTable tab = {};
    if (!seg_end) {                 // a null table: one segment over everything, the scalar lr / weight_decay
        nseg = 1;
        tab.end[0] = n; tab.lr[0] = lr; tab.wd[0] = weight_decay;
    } else {
        OWL_CHECK_ARG(nseg >= 1 && nseg <= OWL_OPT_MAX_SEGS, "owl_adamw_step_ema: 1 <= nseg <= %d, got %d", OWL_OPT_MAX_SEGS, nseg);
        int64_t prev = 0;
        for (int s = 0; s < nseg; s++) {
            OWL_CHECK_ARG(seg_end[s] % 4 == 0, "owl_adamw_step_ema: seg_end[%d] = %lld is not a multiple of 4", s, (long long)seg_end[s]);
            OWL_CHECK_ARG(seg_end[s] > prev, "owl_adamw_step_ema: seg_end must be strictly increasing (seg_end[%d] = %lld after %lld)", s,
                          (long long)seg_end[s], (long long)prev);
            prev = tab.end[s] = seg_end[s];
            tab.lr[s] = seg_lr ? seg_lr[s] : lr;
            tab.wd[s] = seg_wd ? seg_wd[s] : weight_decay;
        }
        OWL_CHECK_ARG(prev == n, "owl_adamw_step_ema: seg_end[nseg-1] = %lld must equal n = %lld", (long long)prev, (long long)n);
    }
    OWL_CHECK_ARG(!(max_norm > 0.f) || (workspace && norm_out), "owl_adamw_step_ema: null pointer (workspace, norm_out: both needed when max_norm > 0)");
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_ema_kernel, dim3(step_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, n, beta1, beta2, eps,
                       bc1, bc2_sqrt, grad_scale, max_norm, (const double*)workspace, (int)sumsq_blocks(n), norm_out, tab, nseg, ema, d, w);
    OWL_LAUNCH_CHECK();
    return 0;
}
