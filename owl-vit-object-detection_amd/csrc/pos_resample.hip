// Position table at another input size than the checkpoint's: U [gh gw + 1, D] (row 1 + y gw + x) = bicubic resample of the native table pos [g0 g0 + 1, D] (HF5:296-332
// `interpolate_pos_encoding` = torch.nn.functional.interpolate(mode="bicubic", align_corners=False) on the [g0, g0, D] patch rows; the class row is
// copied), and its exact adjoint for a trainable table.  Run only by a model built at g != g0 (models.OwlViT); f32 in and out.
// Both kernels evaluate the same per-axis taps (axis_taps below), in plain f32 with contraction off and explicit fmaf, so that the rounding count
// tests/pos_resample_reference.py states is the code's.  Deterministic: no atomics, every sum in a fixed order.
#include "common.h"

#define POS_MAX_GRID 256          // side of either grid (P = 65536: far past the 8192-patch ceiling of owl_spread_labels / owl_postprocess)

__device__ __forceinline__ int floor_div(int a, int b) {          // b > 0
    const int q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// Taps of output index o on one axis.  Source coordinate s = (o + 0.5) g0 / g - 0.5 = num / den in integers, f = floor(s), t = s - f = r / den with
// 0 <= r < den: ONE f32 rounding (the division; r and den are exact).  Taps f - 1 .. f + 2 clamped to [0, g0 - 1]; cubic-convolution weights with
// A = -0.75 in torch's Horner forms (UpSample.h cubic_convolution1 / 2); every constant below is exact in f32.
__device__ __forceinline__ void axis_taps(int o, int g0, int g, int idx[4], float w[4]) {
#pragma clang fp contract(off)
    const int den = 2 * g;
    const int num = (2 * o + 1) * g0 - g;
    const int f = floor_div(num, den);
    const float t = (float)(num - f * den) / (float)den;
    const float x0 = t + 1.0f, u = 1.0f - t, x3 = 2.0f - t;
    w[0] = ((-0.75f * x0 + 3.75f) * x0 - 6.0f) * x0 + 3.0f;
    w[1] = ((1.25f * t - 2.25f) * t) * t + 1.0f;
    w[2] = ((1.25f * u - 2.25f) * u) * u + 1.0f;
    w[3] = ((-0.75f * x3 + 3.75f) * x3 - 6.0f) * x3 + 3.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) idx[i] = min(max(f - 1 + i, 0), g0 - 1);
}

// ---------------------------------------------------------------------------------------------------
// forward: one workgroup per row of U, one thread per 4 columns (16 bytes per lane, the row contiguous across the lanes).  The taps are the
// same in every lane.  out[1 + y g + x] = sum_{i, j} fl(wy_i wx_j) pos[1 + cy_i g0 + cx_j], i outer, j inner, one fmaf per tap.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pos_resample_kernel(const float* __restrict__ pos, float* __restrict__ out, int g0, int gh, int gw, int D) {
#pragma clang fp contract(off)
    const int t = blockIdx.x;
    if (t == 0) {
        for (int c = threadIdx.x * 4; c < D; c += 1024) *(float4*)(out + c) = *(const float4*)(pos + c);
        return;
    }
    int iy[4], ix[4];
    float wy[4], wx[4];
    axis_taps((t - 1) / gw, g0, gh, iy, wy);
    axis_taps((t - 1) % gw, g0, gw, ix, wx);
    for (int c = threadIdx.x * 4; c < D; c += 1024) {
        float4 a = make_float4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float w = wy[i] * wx[j];
                const float4 p = *(const float4*)(pos + (int64_t)(1 + iy[i] * g0 + ix[j]) * D + c);
                a.x = fmaf(w, p.x, a.x); a.y = fmaf(w, p.y, a.y); a.z = fmaf(w, p.z, a.z); a.w = fmaf(w, p.w, a.w);
            }
        }
        *(float4*)(out + (int64_t)t * D + c) = a;
    }
}

OWL_API int owl_pos_resample_hw(void* stream, const float* pos, float* out, int64_t g0, int64_t gh, int64_t gw, int64_t D) {
    OWL_CHECK_ARG(pos && out, "owl_pos_resample: null pointer");
    OWL_CHECK_ARG(g0 >= 1 && g0 <= POS_MAX_GRID && gh >= 1 && gh <= POS_MAX_GRID && gw >= 1 && gw <= POS_MAX_GRID && D >= 8 && D % 8 == 0 && D < (1 << 20),
                  "owl_pos_resample: grids of side 1 .. 256, D a positive multiple of 8");
    hipLaunchKernelGGL(pos_resample_kernel, dim3((unsigned)(gh * gw + 1)), dim3(256), 0, (hipStream_t)stream, pos, out, (int)g0, (int)gh, (int)gw, (int)D);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_pos_resample(void* stream, const float* pos, float* out, int64_t g0, int64_t g, int64_t D) {
    return owl_pos_resample_hw(stream, pos, out, g0, g, g, D);
}

// ---------------------------------------------------------------------------------------------------
// backward, as a gather: one workgroup per row of dpos (= source cell (sy, sx)), one thread per 4 columns.  The output cells whose clamped taps
// touch the cell are a rectangle [y_lo, y_hi] x [x_lo, x_hi] (f is monotone in o; a border cell also takes every tap clamped onto it).  Per axis,
// m(o) = the sum, in tap order, of the weights of o whose clamped tap is this cell -- made once per workgroup into LDS --, then
// dpos[cell] += sum_{y, x} fl(my(y) mx(x)) dU[1 + y g + x], y outer, x inner, ascending, one fmaf per term, and ONE add onto the value already there.
// ---------------------------------------------------------------------------------------------------
// smallest o >= 0 with f(o) >= F:  (2 o + 1) g0 - g >= 2 g F  <=>  2 o + 1 >= q = ceil((2 g F + g) / g0)  <=>  o >= floor(q / 2)
__device__ __forceinline__ int first_with_floor(int F, int g0, int g) {
    const int q = -floor_div(-(2 * g * F + g), g0);
    return max(floor_div(q, 2), 0);
}

__device__ __forceinline__ void touch_range(int s, int g0, int g, int& lo, int& hi) {
    lo = (s == 0) ? 0 : min(first_with_floor(s - 2, g0, g), g);                    // taps f - 1 .. f + 2 reach s: s - 2 <= f <= s + 1
    hi = (s == g0 - 1) ? g - 1 : min(first_with_floor(s + 2, g0, g), g) - 1;
}

__device__ __forceinline__ float axis_weight_on(int o, int s, int g0, int g) {
#pragma clang fp contract(off)
    int idx[4];
    float w[4];
    axis_taps(o, g0, g, idx, w);
    float m = 0.0f;          // (0 + w is exact: k taps on the cell cost k - 1 roundings)
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (idx[i] == s) m += w[i];
    return m;
}

__global__ __launch_bounds__(256) void pos_resample_bwd_kernel(const float* __restrict__ dU, float* __restrict__ dpos, int g0, int gh, int gw, int D) {
#pragma clang fp contract(off)
    __shared__ float s_my[POS_MAX_GRID], s_mx[POS_MAX_GRID];
    const int cell = blockIdx.x;
    if (cell == 0) {
        for (int c = threadIdx.x * 4; c < D; c += 1024) {
            const float4 v = *(const float4*)(dU + c);
            float4 r = *(float4*)(dpos + c);
            r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
            *(float4*)(dpos + c) = r;
        }
        return;
    }
    const int sy = (cell - 1) / g0, sx = (cell - 1) % g0;
    int y_lo, y_hi, x_lo, x_hi;
    touch_range(sy, g0, gh, y_lo, y_hi);
    touch_range(sx, g0, gw, x_lo, x_hi);
    for (int k = y_lo + threadIdx.x; k <= y_hi; k += 256) s_my[k] = axis_weight_on(k, sy, g0, gh);
    for (int k = x_lo + threadIdx.x; k <= x_hi; k += 256) s_mx[k] = axis_weight_on(k, sx, g0, gw);
    __syncthreads();
    for (int c = threadIdx.x * 4; c < D; c += 1024) {
        float4 a = make_float4(0, 0, 0, 0);
        for (int y = y_lo; y <= y_hi; y++) {
            const float my = s_my[y];
            const float* row = dU + (int64_t)(1 + y * gw) * D + c;
            for (int x = x_lo; x <= x_hi; x++) {
                const float m = my * s_mx[x];
                const float4 v = *(const float4*)(row + (int64_t)x * D);
                a.x = fmaf(m, v.x, a.x); a.y = fmaf(m, v.y, a.y); a.z = fmaf(m, v.z, a.z); a.w = fmaf(m, v.w, a.w);
            }
        }
        float4* o = (float4*)(dpos + (int64_t)cell * D + c);
        float4 r = *o;
        r.x += a.x; r.y += a.y; r.z += a.z; r.w += a.w;
        *o = r;
    }
}

OWL_API int owl_pos_resample_bwd_hw(void* stream, const float* dU, float* dpos, int64_t g0, int64_t gh, int64_t gw, int64_t D) {
    OWL_CHECK_ARG(dU && dpos, "owl_pos_resample_bwd: null pointer");
    OWL_CHECK_ARG(g0 >= 1 && g0 <= POS_MAX_GRID && gh >= 1 && gh <= POS_MAX_GRID && gw >= 1 && gw <= POS_MAX_GRID && D >= 8 && D % 8 == 0 && D < (1 << 20),
                  "owl_pos_resample_bwd: grids of side 1 .. 256, D a positive multiple of 8");
    hipLaunchKernelGGL(pos_resample_bwd_kernel, dim3((unsigned)(g0 * g0 + 1)), dim3(256), 0, (hipStream_t)stream, dU, dpos, (int)g0, (int)gh, (int)gw, (int)D);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_pos_resample_bwd(void* stream, const float* dU, float* dpos, int64_t g0, int64_t g, int64_t D) {
    return owl_pos_resample_bwd_hw(stream, dU, dpos, g0, g, g, D);
}
