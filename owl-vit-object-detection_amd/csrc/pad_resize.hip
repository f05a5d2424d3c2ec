// OWLv2's input stage on the device (HF Owlv2ImageProcessorPil): x(1/255) -> pad bottom / right to a square of side S = max(H, W) -> scipy gaussian_filter
// (sigma = max(0, (S/N - 1)/2), "mirror") -> scipy zoom (order 1, "mirror", grid_mode) to N x N -> (x - mean) / std.
//
// Blur and zoom are separable and linear and the pad is a constant, so per channel the stage is A_y P A_x^T with ONE per-axis matrix A = Z G (the bilinear
// rows times the mirrored Gaussian); the taps that land in the pad drop out of the tables (owl_pad_resize_coeffs, host, f64).  That is the shape of the
// Pillow resampler next door (preprocess.hip): per-axis {first, count} bounds, a weight table and two passes.  What differs is float weights, an f32
// intermediate and up to 62 taps, which the fixed-point u8 kernels cannot express.
//
// The evaluation order is a contract (tests/owlv2_input_reference.py counts its roundings; the file is compiled with -ffp-contract=off):
//   h[s][j]   = fmaf(u8 -> f32 (exact), wx[j][t], h) over the kept taps t in ascending order, from 0          (0..255 units)
//   v[i][j]   = fmaf(h[s][j], wy[i][t], v) over the kept rows in ascending order, from 0
//   v         = fmaf(pad255, 1 - wsum_x[j] * wsum_y[i], v)                                                    (pad_value != 0 only)
//   out[c]    = fmaf(v, a_c, b_c), a_c = rescale / std_c, b_c = -mean_c / std_c                               -> f32, or bf16 round-to-nearest-even
// HBM-bound (no MFMA): per image it reads H W 3 B, writes and re-reads the f32 [H, live4, 3] intermediate, writes 3 N N (4 | 2) B.  No atomics, no
// allocation, no host sync.
#include "common.h"

// the 10 int64 words of preprocess.hip's PreDesc; bx / by hold 2 N + 1 ints (the last one `live` = 1 + the last output index with a tap), wx / wy hold
// N ksize weights followed by the N row sums `wsum`; tmp_off in bytes, a multiple of 16
struct PadDesc { const unsigned char* src; long long H, W; const int* bx; const float* wx; long long ksx; const int* by; const float* wy; long long ksy; long long tmp_off; };

#define PR_ROWS 4          // source rows a thread of the horizontal pass takes: the weights of its column are read once for all of them
#define PR_QUAD 4          // adjacent output pixels a thread of the vertical pass takes: 3 x 16-byte loads per tap row, one 16 | 8-byte store per plane

__device__ __forceinline__ int live4_of(int live) { return (live + 3) & ~3; }

// u8 [H, W, 3] -> f32 [H, live4, 3].  Columns in [live, live4) -- and columns below `live` without a tap -- are written as 0: the vertical pass loads whole quads.
__global__ __launch_bounds__(256) void pr_h_kernel(const PadDesc* __restrict__ desc, float* __restrict__ tmp_base, int out_w) {
    const PadDesc d = desc[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * PR_ROWS;
    const int l4 = live4_of(d.bx[2 * out_w]);
    if (x >= l4 || r0 >= d.H) return;
    int xmin = 0, n = 0;
    if (x < out_w) { xmin = d.bx[2 * x]; n = d.bx[2 * x + 1]; }
    const float* k = d.wx + (int64_t)x * d.ksx;
    const int last = (int)d.H - 1;
    const unsigned char* row[PR_ROWS];                         // rows past the image re-read its last one (in bounds) and are not stored
    float acc[PR_ROWS][3];
#pragma unroll
    for (int j = 0; j < PR_ROWS; j++) {
        row[j] = d.src + ((int64_t)min(r0 + j, last) * d.W + xmin) * 3;
        acc[j][0] = acc[j][1] = acc[j][2] = 0.0f;
    }
    for (int t = 0; t < n; t++) {
        const float w = k[t];
#pragma unroll
        for (int j = 0; j < PR_ROWS; j++) {
            acc[j][0] = fmaf((float)row[j][3 * t], w, acc[j][0]);
            acc[j][1] = fmaf((float)row[j][3 * t + 1], w, acc[j][1]);
            acc[j][2] = fmaf((float)row[j][3 * t + 2], w, acc[j][2]);
        }
    }
    float* tmp = (float*)((char*)tmp_base + d.tmp_off);
#pragma unroll
    for (int j = 0; j < PR_ROWS; j++) {
        if (r0 + j > last) break;
        float* o = tmp + ((int64_t)(r0 + j) * l4 + x) * 3;
        o[0] = acc[j][0]; o[1] = acc[j][1]; o[2] = acc[j][2];
    }
}

// f32 [H, live4, 3] -> out [n, 3, out_h, out_w].  A workgroup is 64 quads x 4 output rows: a wave has one output row, so its weights are wave-uniform.
template <bool BF16>
__global__ __launch_bounds__(256) void pr_v_kernel(const PadDesc* __restrict__ desc, const float* __restrict__ tmp_base, void* __restrict__ out,
                                                   const float* __restrict__ norm, float pad255, int out_h, int out_w) {
    const PadDesc d = desc[blockIdx.z];
    const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * PR_QUAD, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x4 >= out_w || y >= out_h) return;
    const int l4 = live4_of(d.bx[2 * out_w]);
    const int ymin = d.by[2 * y], n = d.by[2 * y + 1];
    float acc[PR_QUAD][3];
#pragma unroll
    for (int p = 0; p < PR_QUAD; p++) acc[p][0] = acc[p][1] = acc[p][2] = 0.0f;
    if (x4 < l4) {                                             // both multiples of 4: the whole quad was written by the horizontal pass
        const float* k = d.wy + (int64_t)y * d.ksy;
        const int64_t stride = (int64_t)l4 * 3;
        const float* col = (const float*)((const char*)tmp_base + d.tmp_off) + (int64_t)ymin * stride + (int64_t)x4 * 3;
        for (int t = 0; t < n; t++) {
            const float w = k[t];
            const float4 a = *(const float4*)(col + t * stride), b = *(const float4*)(col + t * stride + 4), c = *(const float4*)(col + t * stride + 8);
            acc[0][0] = fmaf(a.x, w, acc[0][0]); acc[0][1] = fmaf(a.y, w, acc[0][1]); acc[0][2] = fmaf(a.z, w, acc[0][2]);
            acc[1][0] = fmaf(a.w, w, acc[1][0]); acc[1][1] = fmaf(b.x, w, acc[1][1]); acc[1][2] = fmaf(b.y, w, acc[1][2]);
            acc[2][0] = fmaf(b.z, w, acc[2][0]); acc[2][1] = fmaf(b.w, w, acc[2][1]); acc[2][2] = fmaf(c.x, w, acc[2][2]);
            acc[3][0] = fmaf(c.y, w, acc[3][0]); acc[3][1] = fmaf(c.z, w, acc[3][1]); acc[3][2] = fmaf(c.w, w, acc[3][2]);
        }
    }
    if (pad255 != 0.0f) {                                      // the pad's share of the pixel: every weight of the full row sums to 1
        const float sy = d.wy[(int64_t)out_h * d.ksy + y];
        const float* sx = d.wx + (int64_t)out_w * d.ksx;
#pragma unroll
        for (int p = 0; p < PR_QUAD; p++) {
            const float q = sx[min(x4 + p, out_w - 1)] * sy;
            const float r = 1.0f - q;
            acc[p][0] = fmaf(pad255, r, acc[p][0]); acc[p][1] = fmaf(pad255, r, acc[p][1]); acc[p][2] = fmaf(pad255, r, acc[p][2]);
        }
    }
    const int64_t plane = (int64_t)out_h * out_w;
    const bool vec = (out_w % PR_QUAD) == 0;                   // then every quad is whole and its stores are aligned (out is 16-byte aligned)
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a = norm[c], b = norm[3 + c];
        const float v0 = fmaf(acc[0][c], a, b), v1 = fmaf(acc[1][c], a, b), v2 = fmaf(acc[2][c], a, b), v3 = fmaf(acc[3][c], a, b);
        const int64_t o = ((int64_t)blockIdx.z * 3 + c) * plane + (int64_t)y * out_w + x4;
        if (BF16) {
            bf16_t* p = (bf16_t*)out + o;
            if (vec) {
                *(uint2*)p = make_uint2(pack_bf2(v0, v1), pack_bf2(v2, v3));
            } else {
                p[0] = f2bf(v0);
                if (x4 + 1 < out_w) p[1] = f2bf(v1);
                if (x4 + 2 < out_w) p[2] = f2bf(v2);
                if (x4 + 3 < out_w) p[3] = f2bf(v3);
            }
        } else {
            float* p = (float*)out + o;
            if (vec) {
                *(float4*)p = make_float4(v0, v1, v2, v3);
            } else {
                p[0] = v0;
                if (x4 + 1 < out_w) p[1] = v1;
                if (x4 + 2 < out_w) p[2] = v2;
                if (x4 + 3 < out_w) p[3] = v3;
            }
        }
    }
}

OWL_API int owl_preprocess_u8_pad_resize(void* stream, const void* desc, int64_t n_images, int64_t max_h, float* tmp_f32, const float* norm, float pad_value,
                                         void* out, int out_bf16, int64_t out_h, int64_t out_w) {
    OWL_CHECK_ARG(desc && tmp_f32 && norm && out, "owl_preprocess_u8_pad_resize: null pointer");
    OWL_CHECK_ARG(n_images > 0 && n_images < 65536 && max_h > 0 && max_h < 65536 * PR_ROWS && out_h > 0 && out_h < 65536 && out_w > 0 && out_w < 65536,
                  "owl_preprocess_u8_pad_resize: bad sizes n=%lld max_h=%lld out=%lldx%lld", (long long)n_images, (long long)max_h, (long long)out_h, (long long)out_w);
    OWL_CHECK_ARG(((uintptr_t)tmp_f32 & 15) == 0 && ((uintptr_t)out & 15) == 0, "owl_preprocess_u8_pad_resize: tmp_f32 and out must be 16-byte aligned");
    OWL_CHECK_ARG(pad_value == pad_value && pad_value >= 0.0f && pad_value <= 1.0f, "owl_preprocess_u8_pad_resize: pad_value %g outside [0, 1]", (double)pad_value);
    hipStream_t s = (hipStream_t)stream;
    const float pad255 = (float)(255.0 * (double)pad_value);
    const int64_t w4 = (out_w + 3) / 4 * 4;
    hipLaunchKernelGGL(pr_h_kernel, dim3((unsigned)((w4 + 255) / 256), (unsigned)((max_h + PR_ROWS - 1) / PR_ROWS), (unsigned)n_images), dim3(256), 0, s,
                       (const PadDesc*)desc, tmp_f32, (int)out_w);
    OWL_LAUNCH_CHECK();
    const dim3 grid((unsigned)((out_w + 64 * PR_QUAD - 1) / (64 * PR_QUAD)), (unsigned)((out_h + 3) / 4), (unsigned)n_images);
    if (out_bf16)
        hipLaunchKernelGGL((pr_v_kernel<true>), grid, dim3(256), 0, s, (const PadDesc*)desc, tmp_f32, out, norm, pad255, (int)out_h, (int)out_w);
    else
        hipLaunchKernelGGL((pr_v_kernel<false>), grid, dim3(256), 0, s, (const PadDesc*)desc, tmp_f32, out, norm, pad255, (int)out_h, (int)out_w);
    OWL_LAUNCH_CHECK();
    return 0;
}
