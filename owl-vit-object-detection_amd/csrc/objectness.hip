// OWLv2's objectness head, the tail of it: dense2 (D -> 1) forward and its backward fused with dense1's erf-GELU derivative.
// HF: Owlv2ForObjectDetection.objectness_predictor = Owlv2BoxPredictionHead(out_dim=1) on the DETACHED image features:
//     o = dense2(gelu(dense1(gelu(dense0(feats)))))[..., 0].   dense0 / dense1 are GEMM launches (EPI_GELU_BF16 forward, EPI_DGELU_BF16 and the weight-gradient
// route backward); the two kernels here are the one-output forms of box_final_rows_kernel (heads.hip) and box_final_bwd_kernel (backward.hip).
// Compiled with contraction off (build.sh): tests/objectness_reference.py counts one rounding per written operation; the fused steps are named (fmaf).
#include "common.h"

// ---- forward: logits[r] = sum_j h[r, j] w2[j] + b2 ------------------------------------------------------------------------------------------
// Lane l owns elements 8 l .. 8 l + 7 (+ 512 for D > 512) of the row and adds its products in that order (one fmaf chain), the 64 partial sums meet pair
// by pair at distances 32, 16, ..., 1 (wave_sum), then the bias.  A wave walks rows_per_wave rows with its slice of w2 in registers and the next two rows
// requested while one is worked on, as the box tail does: the kernel streams rows x D bf16 once and is bound by that read.
template <int NC>
__global__ __launch_bounds__(256) void objectness_final_rows_kernel(const bf16_t* __restrict__ h, const float* __restrict__ w2, const float* __restrict__ b2,
                                                                    float* logits, int64_t rows, int D, int rows_per_wave) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * rows_per_wave;
    const int64_t row1 = min(rows, row0 + rows_per_wave);
    if (row0 >= row1) return;
    bool act[NC];
    float wr[NC][8];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int k = lane * 8 + 512 * c;
        act[c] = k < D;
        float4 lo = make_float4(0, 0, 0, 0), hi4 = lo;
        if (act[c]) { lo = *(const float4*)(w2 + k); hi4 = *(const float4*)(w2 + k + 4); }
        wr[c][0] = lo.x; wr[c][1] = lo.y; wr[c][2] = lo.z; wr[c][3] = lo.w;
        wr[c][4] = hi4.x; wr[c][5] = hi4.y; wr[c][6] = hi4.z; wr[c][7] = hi4.w;
    }
    const float bias = b2[0];
    struct RowIn { us8 hv[NC]; };
    auto fetch = [&](int64_t r, RowIn& x) {
        r = min(r, row1 - 1);                           // unconditional (the surplus fetches are dropped)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            x.hv[c] = us8{0, 0, 0, 0, 0, 0, 0, 0};
            if (act[c]) x.hv[c] = *(const us8*)(h + r * D + lane * 8 + 512 * c);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto process = [&](int64_t r, const RowIn& x) {
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (act[c]) {
#pragma unroll
                for (int e = 0; e < 8; e++) a = fmaf(bf2f(x.hv[c][e]), wr[c][e], a);
            }
        }
        a = wave_sum(a);
        if (lane == 0) logits[r] = a + bias;
    };
    RowIn x0, x1, x2;
    fetch(row0, x0); fetch(row0 + 1, x1);
    for (int64_t r = row0; r < row1; r += 3) {
        fetch(r + 2, x2); process(r, x0);
        if (r + 1 >= row1) break;
        fetch(r + 3, x0); process(r + 1, x1);
        if (r + 2 >= row1) break;
        fetch(r + 4, x1); process(r + 2, x2);
    }
}

// rows per wave: the box tail's rule (16 at large batch: the weight slice is loaded once per wave; 1 while that would leave CUs idle)
static int64_t objectness_rpw(int64_t rows) {
    const int64_t rpw = (rows + 4095) / 4096;
    return rpw < 1 ? 1 : (rpw > 16 ? 16 : rpw);
}

OWL_API int owl_objectness_final_fwd(void* stream, const void* h_bf16, const float* w2, const float* b2, float* logits, int64_t rows, int64_t D) {
    OWL_CHECK_ARG(h_bf16 && w2 && b2 && logits, "owl_objectness_final_fwd: null pointer");
    OWL_CHECK_ARG(rows >= 1, "owl_objectness_final_fwd: rows >= 1 required (got %lld)", (long long)rows);
    OWL_CHECK_ARG(D % 8 == 0 && D >= 8 && D <= 1024, "owl_objectness_final_fwd: D %% 8 == 0 and 8 <= D <= 1024 required (got %lld)", (long long)D);
    const int64_t rpw = objectness_rpw(rows);
    const dim3 grid((unsigned)((rows + 4 * rpw - 1) / (4 * rpw)));
    if (D <= 512)
        hipLaunchKernelGGL(objectness_final_rows_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)h_bf16, w2, b2, logits, rows, (int)D, (int)rpw);
    else
        hipLaunchKernelGGL(objectness_final_rows_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)h_bf16, w2, b2, logits, rows, (int)D, (int)rpw);
    OWL_LAUNCH_CHECK();
    return 0;
}

// ---- backward: du1 = bf16(g_r w2_j gelu'(u1_rj)) ; dw2_j = sum_r g_r h1_rj ; db2 = sum_r g_r ; colsum_j = sum_r du1_rj (f32, before the bf16 rounding) ----
// One thread owns FOUR consecutive columns (8-byte loads of h1 / u1, 8-byte store of du1; its four dense2 weights live in registers) and walks the
// workgroup's rows four at a time with the next four rows' operands in flight.  Per column the arithmetic and the row order of the sums are those of a
// plain row loop:  o = (g w) gelu'(u);  colsum += o;  dw2 = fmaf(g, h, dw2).  No atomics: every workgroup writes one partial row
// [dw2 (D) | db2, 0, 0, 0 | colsum (D)], which owl_slab_reduce_impl adds up in a fixed order.
__global__ __launch_bounds__(256) void objectness_final_bwd_kernel(const float* __restrict__ dlogits, const bf16_t* __restrict__ h1, const bf16_t* __restrict__ u1,
                                                                   const float* __restrict__ w2, bf16_t* __restrict__ du1, float* __restrict__ part,
                                                                   int64_t rows, int D, int rows_per_block) {
#pragma clang fp contract(off)
    __shared__ float g_s[256];
    const int t = threadIdx.x;
    const int col = 4 * t;
    const bool col_ok = col < D;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block, r_end = min(rows, r_begin + rows_per_block);
    float accw[4] = {0.f, 0.f, 0.f, 0.f};     // dw2
    float accu[4] = {0.f, 0.f, 0.f, 0.f};     // column sums of du1: dense1's bias gradient
    float accb = 0.f;
    float wk[4] = {0.f, 0.f, 0.f, 0.f};
    if (col_ok) {
        const float4 w = *(const float4*)(w2 + col);
        wk[0] = w.x; wk[1] = w.y; wk[2] = w.z; wk[3] = w.w;
    }
    for (int64_t r0 = r_begin; r0 < r_end; r0 += 256) {
        const int64_t r = r0 + t;
        float g = 0.f;
        if (r < r_end) { g = dlogits[r]; accb += g; }
        __syncthreads();
        g_s[t] = g;
        __syncthreads();
        const int nr = (int)min((int64_t)256, r_end - r0);
        if (col_ok) {
            uint2 hn[4], un[4];                          // the NEXT four rows' operands: in flight while these four are computed
            auto fetch = [&](int rr) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int64_t row = r0 + min(rr + j, nr - 1);
                    hn[j] = ld_stream_u2(h1 + row * D + col);
                    un[j] = ld_stream_u2(u1 + row * D + col);
                }
            };
            fetch(0);
            for (int rr = 0; rr < nr; rr += 4) {
                uint2 hq[4], uq[4];
#pragma unroll
                for (int j = 0; j < 4; j++) { hq[j] = hn[j]; uq[j] = un[j]; }
                if (rr + 4 < nr) fetch(rr + 4);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (rr + j >= nr) break;
                    const float d = g_s[rr + j];
                    const float hv[4] = {bf2f(hq[j].x & 0xffff), bf2f(hq[j].x >> 16), bf2f(hq[j].y & 0xffff), bf2f(hq[j].y >> 16)};
                    const float uv[4] = {bf2f(uq[j].x & 0xffff), bf2f(uq[j].x >> 16), bf2f(uq[j].y & 0xffff), bf2f(uq[j].y >> 16)};
                    float o[4];
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const float dh1 = d * wk[c];
                        o[c] = dh1 * dgelu_erf_f(uv[c]);
                        accu[c] += o[c];
                        accw[c] = fmaf(d, hv[c], accw[c]);
                    }
                    uint2 ov; ov.x = pack_bf2(o[0], o[1]); ov.y = pack_bf2(o[2], o[3]);
                    *(uint2*)(du1 + (r0 + rr + j) * D + col) = ov;
                }
            }
        }
    }
    float* mypart = part + (int64_t)blockIdx.x * (2 * D + 4);
    if (col_ok) {
        *(float4*)(mypart + col) = make_float4(accw[0], accw[1], accw[2], accw[3]);
        *(float4*)(mypart + D + 4 + col) = make_float4(accu[0], accu[1], accu[2], accu[3]);
    }
    __shared__ float redb[4];
    accb = wave_sum(accb);
    if ((t & 63) == 0) redb[t >> 6] = accb;
    __syncthreads();
    if (t == 0) *(float4*)(mypart + D) = make_float4(((redb[0] + redb[1]) + redb[2]) + redb[3], 0.f, 0.f, 0.f);
}

// rows per workgroup: the box tail's rule (64 at large batch, down to 8 when that would leave most CUs idle)
static int objectness_bwd_rpb(int64_t rows) {
    const int64_t r = (rows + 511) / 512;
    return (int)(r < 8 ? 8 : (r > 64 ? 64 : r));
}
OWL_API int owl_objectness_final_bwd_blocks(int64_t rows) {
    if (rows < 1) return 0;
    const int rpb = objectness_bwd_rpb(rows);
    return (int)((rows + rpb - 1) / rpb);
}

// partials: f32 workspace [owl_objectness_final_bwd_blocks(rows)][2 D + 4].  dw2_db2: f32 [D + 4] = dw2 [D], db2, three zeros (the reducer works in
// quads).  du1_colsum (optional, [D]): the column sums of du1.  All three are WRITTEN, not accumulated into.
OWL_API int owl_objectness_final_bwd(void* stream, const float* dlogits, const void* h1_bf16, const void* u1_bf16, const float* w2, void* du1_bf16,
                                     float* partials, float* dw2_db2, int64_t rows, int64_t D, float* du1_colsum) {
    OWL_CHECK_ARG(dlogits && h1_bf16 && u1_bf16 && w2 && du1_bf16 && partials && dw2_db2, "owl_objectness_final_bwd: null pointer");
    OWL_CHECK_ARG(rows >= 1, "owl_objectness_final_bwd: rows >= 1 required (got %lld)", (long long)rows);
    OWL_CHECK_ARG(D % 8 == 0 && D >= 8 && D <= 1024, "owl_objectness_final_bwd: D %% 8 == 0 and 8 <= D <= 1024 required (got %lld)", (long long)D);
    const int rpb = objectness_bwd_rpb(rows);
    const int nblk = (int)((rows + rpb - 1) / rpb);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(objectness_final_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, s, dlogits, (const bf16_t*)h1_bf16, (const bf16_t*)u1_bf16, w2,
                       (bf16_t*)du1_bf16, partials, rows, (int)D, rpb);
    OWL_LAUNCH_CHECK();
    int rc = owl_slab_reduce_impl(s, partials, dw2_db2, D + 4, 2 * D + 4, nblk, 0);
    if (rc || !du1_colsum) return rc;
    return owl_slab_reduce_impl(s, partials + D + 4, du1_colsum, D, 2 * D + 4, nblk, 0);
}
