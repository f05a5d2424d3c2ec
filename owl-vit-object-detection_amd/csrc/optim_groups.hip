// Grouped, clipped AdamW over the flat trainable bucket: what torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with several parameter
// groups do, in two launches.  Sibling of optim.hip (adamw_kernel stays the one-group, unclipped path; this file is compiled with the same flags).
//   grad_sumsq_kernel     one read of the gradient bucket -> one f64 partial sum of squares per workgroup (fixed order, no atomics)
//   adamw_grouped_kernel  every workgroup adds the partials in ONE fixed order (identical bits everywhere), forms the clip coefficient and runs
//                         adamw_kernel's arithmetic with lr / weight_decay taken per segment of the bucket from a table passed by value
#include "optim_common.h"          // SegTable, block_sum_f64, sumsq_blocks: shared with optim_ema.hip

__device__ __forceinline__ double sq_acc(double acc, const float4& x) {
    acc = fma((double)x.x, (double)x.x, acc);
    acc = fma((double)x.y, (double)x.y, acc);
    acc = fma((double)x.z, (double)x.z, acc);
    return fma((double)x.w, (double)x.w, acc);
}

// HBM-bound: one read of g.  The grid depends on n alone and every thread adds its elements in ascending order into an f64 accumulator (the
// four-trip unrolling only puts four loads in flight; the additions keep the order of the one-trip loop), so the same g gives the same bits.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
    __shared__ double wsum[4];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    double acc = 0.0;
    for (; i + 3 * stride < n; i += 4 * stride) {
        const float4 a = *(const float4*)(g + i), b = *(const float4*)(g + i + stride), c = *(const float4*)(g + i + 2 * stride),
                     d = *(const float4*)(g + i + 3 * stride);
        acc = sq_acc(sq_acc(sq_acc(sq_acc(acc, a), b), c), d);
    }
    for (; i < n; i += stride) acc = sq_acc(acc, *(const float4*)(g + i));
    const double tot = block_sum_f64(acc, wsum);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void adamw_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, bf16_t* __restrict__ p_bf16, int64_t n, float b1, float b2,
                                                            float eps, float bc1, float bc2_sqrt, float grad_scale, float max_norm,
                                                            const double* __restrict__ partials, int npart, float* __restrict__ norm_out,
                                                            const SegTable tab, int nseg) {
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
        float pa[4] = {pv.x, pv.y, pv.z, pv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float gg = ga[e] * grad_scale * coef;     // the rest is adamw_kernel's expression sequence: coef == 1 gives its bits
            pa[e] *= (1.f - lr * wd);                       // decoupled weight decay
            ma[e] = b1 * ma[e] + (1.f - b1) * gg;
            va[e] = b2 * va[e] + (1.f - b2) * gg * gg;
            const float denom = sqrtf(va[e]) / bc2_sqrt + eps;
            pa[e] -= (lr / bc1) * (ma[e] / denom);
        }
        *(float4*)(p + i) = make_float4(pa[0], pa[1], pa[2], pa[3]);
        *(float4*)(m + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
        *(float4*)(v + i) = make_float4(va[0], va[1], va[2], va[3]);
        if (p_bf16) {
            uint2 o; o.x = pack_bf2(pa[0], pa[1]); o.y = pack_bf2(pa[2], pa[3]);
            *(uint2*)(p_bf16 + i) = o;
        }
    }
}

OWL_API int owl_grad_norm_workspace_bytes(int64_t n, int64_t* bytes) {
    OWL_CHECK_ARG(bytes, "owl_grad_norm_workspace_bytes: null pointer (bytes)");
    OWL_CHECK_ARG(n > 0 && n % 4 == 0, "owl_grad_norm_workspace_bytes: n must be positive and n %% 4 == 0");
    *bytes = sumsq_blocks(n) * (int64_t)sizeof(double);
    return 0;
}

OWL_API int owl_grad_sumsq(void* stream, const float* g, int64_t n, void* workspace) {
    OWL_CHECK_ARG(g && workspace, "owl_grad_sumsq: null pointer (g, workspace)");
    OWL_CHECK_ARG(n > 0 && n % 4 == 0, "owl_grad_sumsq: n must be positive and n %% 4 == 0");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)sumsq_blocks(n)), dim3(256), 0, (hipStream_t)stream, g, n, (double*)workspace);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_adamw_step_grouped(void* stream, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, int64_t step, float grad_scale, const int64_t* seg_end,
                                   const float* seg_lr, const float* seg_wd, int nseg, float max_norm, const void* workspace, float* norm_out) {
    OWL_CHECK_ARG(p && g && m && v, "owl_adamw_step_grouped: null pointer (p, g, m, v)");
    OWL_CHECK_ARG(seg_end, "owl_adamw_step_grouped: null pointer (seg_end: host array of nseg entries)");
    OWL_CHECK_ARG(n > 0 && n % 4 == 0, "owl_adamw_step_grouped: n must be positive and n %% 4 == 0");
    OWL_CHECK_ARG(step >= 1, "owl_adamw_step_grouped: step >= 1");
    OWL_CHECK_ARG(nseg >= 1 && nseg <= OWL_OPT_MAX_SEGS, "owl_adamw_step_grouped: 1 <= nseg <= %d, got %d", OWL_OPT_MAX_SEGS, nseg);
    SegTable tab = {};
    int64_t prev = 0;
    for (int s = 0; s < nseg; s++) {
        OWL_CHECK_ARG(seg_end[s] % 4 == 0, "owl_adamw_step_grouped: seg_end[%d] = %lld is not a multiple of 4", s, (long long)seg_end[s]);
        OWL_CHECK_ARG(seg_end[s] > prev, "owl_adamw_step_grouped: seg_end must be strictly increasing (seg_end[%d] = %lld after %lld)", s,
                      (long long)seg_end[s], (long long)prev);
        prev = tab.end[s] = seg_end[s];
        tab.lr[s] = seg_lr ? seg_lr[s] : lr;                 // a null table: the scalar argument for every segment
        tab.wd[s] = seg_wd ? seg_wd[s] : weight_decay;
    }
    OWL_CHECK_ARG(prev == n, "owl_adamw_step_grouped: seg_end[nseg-1] = %lld must equal n = %lld", (long long)prev, (long long)n);
    OWL_CHECK_ARG(!(max_norm > 0.f) || (workspace && norm_out),
                  "owl_adamw_step_grouped: null pointer (workspace, norm_out: both needed when max_norm > 0)");
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(adamw_grouped_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, n, beta1,
                       beta2, eps, bc1, bc2_sqrt, grad_scale, max_norm, (const double*)workspace, (int)sumsq_blocks(n), norm_out, tab, nseg);
    OWL_LAUNCH_CHECK();
    return 0;
}
