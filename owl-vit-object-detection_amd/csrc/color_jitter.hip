// Photometric half of the train-time augmentation: brightness, contrast, saturation (and grayscale = saturation 0) per TILE of the device resampler,
// bit-exact against Pillow's ImageEnhance on the tile's resized cell:  resize(box=) -> [transpose] -> ImageEnhance.X(cell).enhance(f) ... -> paste.
//
//   luma   Image.convert("L"):     L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
//   blend  Image.blend(A, B, f):   v = f32(a) + fl32(f32(f) * f32(b - a)), TWO roundings;  v <= 0 -> 0, v >= 255 -> 255, else trunc(v)
//                                  (for 0 <= f <= 1 Pillow skips the clip: v lies in [0, 255] there, so the one form serves both of its branches)
//   Brightness(f) = blend(0, c, f);  Color(f) = blend(L, c, f) per channel;  Contrast(f) = blend(m, c, f), m = int(mean(L) + 0.5) = (2 sum L + n) / (2 n)
//                                  over the n = cw x ch pixels of the cell AS THEY ARE when the op is reached (after the ops that precede it in the tile's order)
//
// A fused multiply-add rounds once and differs from Pillow on 5 538 of the 65 536 x 52 (a, b, f) triples it was checked on: this file is compiled with
// -ffp-contract=off (build.sh) AND names the two roundings.  A factor of exactly 1 is the identity by the arithmetic (a + 1 (b - a) = b): such an op is skipped,
// the contrast sum included.
//
// Three launches.  (1) The horizontal pass as it is (preprocess.hip).  (2) The vertical pass, which stores the clipped u8 level of every channel at its FINAL
// position (cell origin and flip applied) in the element of `out` that will hold its value -- the output tensor is its own canvas, so the workspace holds no
// pixels -- and, for a tile with fc != 1, leaves one integer partial sum of L per workgroup (after the ops that precede contrast).  (3) The colour pass, same
// grid: adds the tile's partials (64-bit; integers, so any order gives the same bits; no atomics), forms m, applies the ops in the tile's order to the levels
// it reads back, looks them up in the normalisation table and stores f32 | bf16 over them.  A pixel's three elements are read and rewritten by one thread.
#include "preprocess_tiles.h"

__device__ __forceinline__ int cj_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int cj_blend8(int a, int b, float f) {
    const float v = __fadd_rn((float)a, __fmul_rn(f, (float)(b - a)));
    return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v);
}

// op 0 = brightness, 1 = contrast, 2 = saturation; the k-th op of order 0..5 = itertools.permutations("bcs")[order][k], 2 bits each
__device__ __forceinline__ int cj_op(int order, int k) {
    const unsigned long long perms = 36ull | (24ull << 6) | (33ull << 12) | (9ull << 18) | (18ull << 24) | (6ull << 30);      // bcs bsc cbs csb sbc scb
    return (int)(perms >> (6 * order + 2 * k)) & 3;
}

struct CjTile { float f[3]; int order; };
__device__ __forceinline__ float cj_factor(const CjTile& c, int op) { return op == 0 ? c.f[0] : (op == 1 ? c.f[1] : c.f[2]); }

__device__ __forceinline__ CjTile cj_load(const float* __restrict__ color, int tile) {
    const float4 c = ((const float4*)color)[tile];
    CjTile t;
    t.f[0] = c.x; t.f[1] = c.y; t.f[2] = c.z;
    t.order = min(5, max(0, (int)c.w));                        // (the host refuses anything else: preprocess.check_color)
    return t;
}

__device__ __forceinline__ void cj_apply(int op, float f, int m, int& r, int& g, int& b) {
    if (f == 1.0f) return;
    if (op == 0) {
        r = cj_blend8(0, r, f); g = cj_blend8(0, g, f); b = cj_blend8(0, b, f);
    } else if (op == 1) {
        r = cj_blend8(m, r, f); g = cj_blend8(m, g, f); b = cj_blend8(m, b, f);
    } else {
        const int L = cj_luma(r, g, b);
        r = cj_blend8(L, r, f); g = cj_blend8(L, g, f); b = cj_blend8(L, b, f);
    }
}

// all 256 threads call it; the total is returned to every thread
__device__ __forceinline__ unsigned long long cj_block_sum(unsigned long long v) {
    __shared__ unsigned long long s_part[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// partial[(tile * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x]: written by the workgroups inside the cell of a tile with fc != 1, read for exactly those
template <bool BF16>
__global__ __launch_bounds__(256) void cj_tile_v_kernel(const TileDesc* __restrict__ desc, const float* __restrict__ color, const unsigned char* __restrict__ tmp_base,
                                                        void* __restrict__ out, unsigned* __restrict__ partial, int out_h, int out_w) {
    const TileDesc d = desc[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * TILE_ROWS;
    if ((long long)blockIdx.x * 256 >= d.cw || y0 >= d.ch) return;                  // the whole workgroup: the ones that stay meet at a barrier
    const CjTile c = cj_load(color, blockIdx.z);
    const bool contrast = c.f[1] != 1.0f;
    unsigned lsum = 0;                                                               // <= 4 x 255 per thread, 261 120 per workgroup
    if (x < d.cw) {
        const int64_t stride = d.cw * 3, plane = (int64_t)out_h * out_w;
        const int ox = (int)d.x0 + (d.flip ? (int)d.cw - 1 - x : x);
        for (int y = y0; y < min(y0 + TILE_ROWS, (int)d.ch); y++) {
            const int ymin = d.by[2 * y] - (int)d.y_first, n = d.by[2 * y + 1];
            const int* k = d.ky + (int64_t)y * d.ksy;
            const unsigned char* col = tmp_base + d.tmp_off + (int64_t)ymin * stride + x * 3;
            int s0 = 1 << (PIL_PRECISION_BITS - 1), s1 = s0, s2 = s0;
            for (int t = 0; t < n; t++) {
                const int w = k[t];
                s0 += (int)col[t * stride] * w;
                s1 += (int)col[t * stride + 1] * w;
                s2 += (int)col[t * stride + 2] * w;
            }
            int r = pil_clip8(s0), g = pil_clip8(s1), b = pil_clip8(s2);
            const int64_t o = d.b * 3 * plane + (d.y0 + y) * out_w + ox;
            if (BF16) {
                bf16_t* p = (bf16_t*)out;
                p[o] = (bf16_t)r; p[plane + o] = (bf16_t)g; p[2 * plane + o] = (bf16_t)b;
            } else {
                unsigned* p = (unsigned*)out;
                p[o] = (unsigned)r; p[plane + o] = (unsigned)g; p[2 * plane + o] = (unsigned)b;
            }
            if (contrast) {
                for (int i = 0; i < 3; i++) {
                    const int op = cj_op(c.order, i);
                    if (op == 1) break;
                    cj_apply(op, cj_factor(c, op), 0, r, g, b);
                }
                lsum += (unsigned)cj_luma(r, g, b);
            }
        }
    }
    if (contrast) {                                                                  // uniform over the workgroup
        const unsigned long long tot = cj_block_sum(lsum);
        if (threadIdx.x == 0) partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (unsigned)tot;
    }
}

template <bool BF16>
__global__ __launch_bounds__(256) void cj_tile_color_kernel(const TileDesc* __restrict__ desc, const float* __restrict__ color, const float* __restrict__ lut,
                                                            void* out, const unsigned* __restrict__ partial, int out_h, int out_w) {
    const TileDesc d = desc[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * TILE_ROWS;
    if ((long long)blockIdx.x * 256 >= d.cw || y0 >= d.ch) return;
    const CjTile c = cj_load(color, blockIdx.z);
    int m = 0;
    if (c.f[1] != 1.0f) {
        const int px = min((int)((d.cw + 255) / 256), (int)gridDim.x), py = min((int)((d.ch + TILE_ROWS - 1) / TILE_ROWS), (int)gridDim.y);   // (a cell lies inside the canvas)
        const unsigned* p = partial + (int64_t)blockIdx.z * gridDim.y * gridDim.x;
        unsigned long long t = 0;
        for (int i = threadIdx.x; i < px * py; i += 256) t += p[(i / px) * gridDim.x + (i % px)];
        const unsigned long long tot = cj_block_sum(t), n = (unsigned long long)(d.cw * d.ch);
        m = (int)((2 * tot + n) / (2 * n));
    }
    if (x >= d.cw) return;
    const int64_t plane = (int64_t)out_h * out_w;
    const int op0 = cj_op(c.order, 0), op1 = cj_op(c.order, 1), op2 = cj_op(c.order, 2);
    for (int y = y0; y < min(y0 + TILE_ROWS, (int)d.ch); y++) {
        const int64_t o = d.b * 3 * plane + (d.y0 + y) * out_w + d.x0 + x;           // final positions: the flip went into the vertical pass's store
        int r, g, b;
        if (BF16) {
            const bf16_t* p = (const bf16_t*)out;
            r = p[o]; g = p[plane + o]; b = p[2 * plane + o];
        } else {
            const unsigned* p = (const unsigned*)out;
            r = (int)p[o]; g = (int)p[plane + o]; b = (int)p[2 * plane + o];
        }
        r &= 255; g &= 255; b &= 255;                                                // (they are levels; keeps the table index in range whatever `out` held)
        cj_apply(op0, cj_factor(c, op0), m, r, g, b);
        cj_apply(op1, cj_factor(c, op1), m, r, g, b);
        cj_apply(op2, cj_factor(c, op2), m, r, g, b);
        const float v0 = lut[r], v1 = lut[256 + g], v2 = lut[512 + b];
        if (BF16) {
            bf16_t* p = (bf16_t*)out;
            p[o] = f2bf(v0); p[plane + o] = f2bf(v1); p[2 * plane + o] = f2bf(v2);
        } else {
            float* p = (float*)out;
            p[o] = v0; p[plane + o] = v1; p[2 * plane + o] = v2;
        }
    }
}

static int64_t cj_workspace_bytes(int64_t n_tiles, int64_t out_h, int64_t out_w) {
    const int64_t gx = (out_w + 255) / 256, gy = (out_h + TILE_ROWS - 1) / TILE_ROWS;
    return (n_tiles * gx * gy * (int64_t)sizeof(unsigned) + 255) / 256 * 256;      // one partial per workgroup of the vertical pass
}

OWL_API int owl_preprocess_color_workspace_bytes(int64_t n_tiles, int64_t out_h, int64_t out_w, int64_t* bytes) {
    OWL_CHECK_ARG(bytes, "owl_preprocess_color_workspace_bytes: null pointer");
    OWL_CHECK_ARG(n_tiles > 0 && n_tiles < 65536 && out_h > 0 && out_h < 65536 && out_w > 0 && out_w < 65536,
                  "owl_preprocess_color_workspace_bytes: bad sizes tiles=%lld out=%lldx%lld", (long long)n_tiles, (long long)out_h, (long long)out_w);
    *bytes = cj_workspace_bytes(n_tiles, out_h, out_w);
    return 0;
}

OWL_API int owl_preprocess_u8_tiles_color(void* stream, const void* desc, const float* color, int64_t n_tiles, int64_t max_rows, unsigned char* tmp,
                                          void* workspace, int64_t workspace_bytes, const float* lut, void* out, int out_bf16, int64_t n_out, int64_t out_h,
                                          int64_t out_w) {
    OWL_CHECK_ARG(desc && color && tmp && workspace && lut && out, "owl_preprocess_u8_tiles_color: null pointer");
    OWL_CHECK_ARG(n_tiles > 0 && n_tiles < 65536 && max_rows > 0 && max_rows < 65536 && n_out > 0 && n_out <= n_tiles && out_h > 0 && out_h < 65536 && out_w > 0 && out_w < 65536,
                  "owl_preprocess_u8_tiles_color: bad sizes tiles=%lld max_rows=%lld n_out=%lld out=%lldx%lld", (long long)n_tiles, (long long)max_rows,
                  (long long)n_out, (long long)out_h, (long long)out_w);
    OWL_CHECK_ARG(workspace_bytes >= cj_workspace_bytes(n_tiles, out_h, out_w), "owl_preprocess_u8_tiles_color: workspace of %lld bytes, need %lld (owl_preprocess_color_workspace_bytes)",
                  (long long)workspace_bytes, (long long)cj_workspace_bytes(n_tiles, out_h, out_w));
    OWL_CHECK_ARG(((uintptr_t)color & 15) == 0 && ((uintptr_t)workspace & 3) == 0, "owl_preprocess_u8_tiles_color: color must be 16-byte, workspace 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int rc = pp_tile_h_launch(s, (const TileDesc*)desc, n_tiles, max_rows, tmp, out_w);
    if (rc != 0) return rc;
    const dim3 grid((unsigned)((out_w + 255) / 256), (unsigned)((out_h + TILE_ROWS - 1) / TILE_ROWS), (unsigned)n_tiles), block(256);
    if (out_bf16)
        hipLaunchKernelGGL((cj_tile_v_kernel<true>), grid, block, 0, s, (const TileDesc*)desc, color, tmp, out, (unsigned*)workspace, (int)out_h, (int)out_w);
    else
        hipLaunchKernelGGL((cj_tile_v_kernel<false>), grid, block, 0, s, (const TileDesc*)desc, color, tmp, out, (unsigned*)workspace, (int)out_h, (int)out_w);
    OWL_LAUNCH_CHECK();
    if (out_bf16)
        hipLaunchKernelGGL((cj_tile_color_kernel<true>), grid, block, 0, s, (const TileDesc*)desc, color, lut, out, (const unsigned*)workspace, (int)out_h, (int)out_w);
    else
        hipLaunchKernelGGL((cj_tile_color_kernel<false>), grid, block, 0, s, (const TileDesc*)desc, color, lut, out, (const unsigned*)workspace, (int)out_h, (int)out_w);
    OWL_LAUNCH_CHECK();
    return 0;
}
