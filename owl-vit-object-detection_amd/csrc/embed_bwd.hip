// The backward below encoder layer 0 -- run only when backbone.embeddings is trainable (models.OwlViT(trainable=...)) -- and the strided slab reducer its
// weight gradient needs at patch sizes whose 3 p p is no multiple of 8.  Reference: the autograd forms of HF5:282-288 (Conv2d k = s = patch, no bias) and
// HF5:336-343 (class token + position embeddings).  Deterministic like the rest of the backward: no atomics, every sum in a fixed order.
#include "common.h"

// ---------------------------------------------------------------------------------------------------
// Backward below encoder layer 0 (only when backbone.embeddings is trainable; HF5:282-288, 336-343).
// embed_bwd: dx [B, Tp, D] f32 = d(embeddings output) ->
//   dpos[t, :] += sum_b dx[b, t, :] (t < T),  dcls += sum_b dx[b, 0, :],  dE[b * P + p, :] = bf16(dx[b, 1 + p, :]) (the dY operand of the
//   patch-embedding weight gradient).  One thread owns 8 columns of one token for the whole batch: the sum over b runs in index order in its registers
//   (no atomics, no second pass), every access is 16 bytes per lane, pad rows t >= T are never touched.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dpos, float* __restrict__ dcls,
                                                        bf16_t* __restrict__ dE, int B, int T, int64_t Tp, int D) {
#pragma clang fp contract(off)
    const int groups = D >> 3;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)T * groups) return;
    const int t = (int)(idx / groups), c = (int)(idx % groups) * 8;
    const int64_t P = T - 1;
    float4 a0 = make_float4(0, 0, 0, 0), a1 = a0;
    for (int b = 0; b < B; b++) {
        const float* src = dx + ((int64_t)b * Tp + t) * D + c;
        const float4 v0 = ld_stream_f4(src), v1 = ld_stream_f4(src + 4);
        a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
        a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
        if (t > 0) *(uint4*)(dE + ((int64_t)b * P + (t - 1)) * D + c) = make_uint4(pack_bf2(v0.x, v0.y), pack_bf2(v0.z, v0.w), pack_bf2(v1.x, v1.y), pack_bf2(v1.z, v1.w));
    }
    float4* o = (float4*)(dpos + (int64_t)t * D + c);
    float4 r0 = o[0], r1 = o[1];
    r0.x += a0.x; r0.y += a0.y; r0.z += a0.z; r0.w += a0.w; r1.x += a1.x; r1.y += a1.y; r1.z += a1.z; r1.w += a1.w;
    o[0] = r0; o[1] = r1;
    if (t == 0) {
        float4* oc = (float4*)(dcls + c);
        float4 c0 = oc[0], c1 = oc[1];
        c0.x += a0.x; c0.y += a0.y; c0.z += a0.z; c0.w += a0.w; c1.x += a1.x; c1.y += a1.y; c1.z += a1.z; c1.w += a1.w;
        oc[0] = c0; oc[1] = c1;
    }
}

OWL_API int owl_embed_bwd(void* stream, const float* dx, float* dpos, float* dcls, void* dE_bf16, int64_t B, int64_t T, int64_t Tp, int64_t D) {
    OWL_CHECK_ARG(dx && dpos && dcls && dE_bf16, "owl_embed_bwd: null pointer");
    OWL_CHECK_ARG(B >= 1 && T >= 2 && Tp >= T && D >= 8 && D % 8 == 0 && B < (1 << 30) && T < (1 << 30) && D < (1 << 30), "owl_embed_bwd: B >= 1, 2 <= T <= Tp, D a positive multiple of 8");
    const int64_t n = T * (D / 8);
    hipLaunchKernelGGL(embed_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, dpos, dcls, (bf16_t*)dE_bf16, (int)B, (int)T, Tp, (int)D);
    OWL_LAUNCH_CHECK();
    return 0;
}

// im2row of the bf16 image [B, 3, H, W] in the conv weight's own column order: out[(b * gh + gy) * gw + gx][(c * ps + i) * ps + j] =
// image[b][c][gy * ps + i][gx * ps + j] (gh = H / ps, gw = W / ps), row stride ld >= 3 ps^2 (columns past 3 ps^2 are left alone) = the X operand of the
// patch-embedding weight gradient.  V bf16 per lane: 8 (16 bytes) where the patch size is a multiple of 8, else 2 (a 14-pixel patch row is 4-byte aligned only).
template <int V>
__global__ __launch_bounds__(256) void im2row_kernel(const bf16_t* __restrict__ img, bf16_t* __restrict__ out, int64_t rows, int H, int W, int ps, int64_t ld) {
    const int per_row = 3 * ps * (ps / V);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * per_row) return;
    const int64_t row = idx / per_row;
    const int k = (int)(idx % per_row) * V;                  // column (c * ps + i) * ps + j, j a multiple of V
    const int j = k % ps, ci = k / ps, i = ci % ps, c = ci / ps;
    const int gw = W / ps, gh = H / ps;
    const int gx = (int)(row % gw), gy = (int)((row / gw) % gh);
    const int64_t b = row / ((int64_t)gh * gw);
    const bf16_t* src = img + ((b * 3 + c) * H + (int64_t)gy * ps + i) * W + (int64_t)gx * ps + j;
    bf16_t* dst = out + row * ld + k;
    if constexpr (V == 8) *(uint4*)dst = *(const uint4*)src;
    else *(unsigned*)dst = *(const unsigned*)src;
}

OWL_API int owl_im2row_bf16_hw(void* stream, const void* image_bf16, void* out_bf16, int64_t ld_out, int64_t B, int64_t H, int64_t W, int64_t ps) {
    OWL_CHECK_ARG(image_bf16 && out_bf16, "owl_im2row_bf16: null pointer");
    OWL_CHECK_ARG(B >= 1 && ps >= 2 && ps % 2 == 0 && ps <= 64 && H >= ps && H % ps == 0 && H <= 8192 && W >= ps && W % ps == 0 && W <= 8192 && B < (1 << 20),
                  "owl_im2row_bf16: even patch size 2 .. 64 that divides the image size");
    OWL_CHECK_ARG(ld_out >= 3 * ps * ps && ld_out % 8 == 0, "owl_im2row_bf16: ld_out >= 3 ps^2 and a multiple of 8");
    const int64_t rows = B * (H / ps) * (W / ps);
    if (ps % 8 == 0) {          // (then W % 8 == 0 as well: every 16-byte piece is aligned)
        const int64_t n = rows * 3 * ps * (ps / 8);
        hipLaunchKernelGGL(im2row_kernel<8>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)image_bf16, (bf16_t*)out_bf16, rows, (int)H, (int)W, (int)ps, ld_out);
    } else {
        const int64_t n = rows * 3 * ps * (ps / 2);
        hipLaunchKernelGGL(im2row_kernel<2>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)image_bf16, (bf16_t*)out_bf16, rows, (int)H, (int)W, (int)ps, ld_out);
    }
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_im2row_bf16(void* stream, const void* image_bf16, void* out_bf16, int64_t ld_out, int64_t B, int64_t S, int64_t ps) {
    return owl_im2row_bf16_hw(stream, image_bf16, out_bf16, ld_out, B, S, S, ps);
}

// out[r][c] (+)= sum_{s < nsplit} slabs[s * slab_stride + r * ld_slab + c], c < cols <= ld_slab: the slab reduction for a split-K product whose slabs carry pad
// columns (a weight gradient with an inner size that is no multiple of 8: the 3 * 14 * 14 = 588 columns of L/14's patch embedding).  Splits are added in index order.
__global__ __launch_bounds__(256) void slab_reduce_rows_kernel(const float* __restrict__ slabs, float* __restrict__ out, int64_t rows, int cols, int64_t ld_slab,
                                                               int64_t slab_stride, int nsplit, int accumulate) {
    const int q = cols >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * q) return;
    const int64_t r = idx / q;
    const int c = (int)(idx % q) * 4;
    const float* src = slabs + r * ld_slab + c;
    float4 a = *(const float4*)src;
    for (int s = 1; s < nsplit; s++) { const float4 v = *(const float4*)(src + (int64_t)s * slab_stride); a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    float4* o = (float4*)(out + r * cols + c);
    if (accumulate) { const float4 v = *o; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    *o = a;
}

OWL_API int owl_slab_reduce_rows(void* stream, const float* slabs, float* out, int64_t rows, int64_t cols, int64_t ld_slab, int64_t slab_stride, int nsplit, int accumulate) {
    OWL_CHECK_ARG(slabs && out && rows > 0 && cols > 0 && cols % 4 == 0 && cols < (1 << 30) && ld_slab >= cols && ld_slab % 4 == 0 && slab_stride >= rows * ld_slab && nsplit >= 1,
                  "owl_slab_reduce_rows: bad args (cols, ld_slab %% 4 == 0, ld_slab >= cols, slab_stride >= rows * ld_slab)");
    const int64_t n = rows * (cols / 4);
    OWL_CHECK_ARG((n + 255) / 256 < (1LL << 31), "owl_slab_reduce_rows: too large");
    hipLaunchKernelGGL(slab_reduce_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, slabs, out, rows, (int)cols, ld_slab, slab_stride, nsplit, accumulate);
    OWL_LAUNCH_CHECK();
    return 0;
}
