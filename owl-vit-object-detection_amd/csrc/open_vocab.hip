// Open-vocabulary class head, forward only: HF's OwlViTClassPredictionHead over query banks that differ per image (text prompts or image exemplars).
//   logit[b, p, q] = (e^_p . q^_{b,q} + shift_p) * scale_p,   e^ = e / (|e| + 1e-6),  q^ = Q / (|Q| + 1e-6)        (HF's epsilon placement)
//   shift_p = w_shift . f_p + b_shift,   scale_p = elu(w_scale . f_p + b_scale) + 1;   finfo(f32).min where mask[b, q] == 0
// A file of its own (compiled with contraction off, csrc/build.sh): the evaluation order below is the one tests/open_vocab_reference.py bounds, and
// the fine-tuning head's kernels (heads.hip, class_head_wide.hip) keep their code and their bits.
#include "common.h"
#include <float.h>

#define OV_MAX_QUERIES 4096
#define OV_MAX_PATCHES 8192        // config.MAX_PATCHES

// ---- pre-pass: shift and scale of every row, once ---------------------------------------------------------------------------------------------
// One wave per row.  Lane l takes the 8-element chunks l, l + 64, ... of the row (bf16 widened to f32, one FMA per element in ascending order),
// the 64 lane sums meet in wave_sum's xor tree: a fixed order, the same for every row.  rowstats[row] = (shift, scale); every query block of the
// main kernel reads these bits.
__global__ __launch_bounds__(256) void logit_rowstats_kernel(const bf16_t* __restrict__ feats, const float* __restrict__ w_shift,
                                                             const float* __restrict__ w_scale, const float* __restrict__ b_shift,
                                                             const float* __restrict__ b_scale, float* rowstats, int64_t rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                               // (whole wave; no barrier in this kernel)
    const bf16_t* f = feats + row * D;
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < (D >> 3); c += 64) {
        const uint4 u = *(const uint4*)(f + c * 8);
        const float4 a0 = *(const float4*)(w_shift + c * 8), a1 = *(const float4*)(w_shift + c * 8 + 4);
        const float4 c0 = *(const float4*)(w_scale + c * 8), c1 = *(const float4*)(w_scale + c * 8 + 4);
        const float x0 = __uint_as_float(u.x << 16), x1 = __uint_as_float(u.x & 0xffff0000u);
        const float x2 = __uint_as_float(u.y << 16), x3 = __uint_as_float(u.y & 0xffff0000u);
        const float x4 = __uint_as_float(u.z << 16), x5 = __uint_as_float(u.z & 0xffff0000u);
        const float x6 = __uint_as_float(u.w << 16), x7 = __uint_as_float(u.w & 0xffff0000u);
        s1 = fmaf(x0, a0.x, s1); s1 = fmaf(x1, a0.y, s1); s1 = fmaf(x2, a0.z, s1); s1 = fmaf(x3, a0.w, s1);
        s1 = fmaf(x4, a1.x, s1); s1 = fmaf(x5, a1.y, s1); s1 = fmaf(x6, a1.z, s1); s1 = fmaf(x7, a1.w, s1);
        s2 = fmaf(x0, c0.x, s2); s2 = fmaf(x1, c0.y, s2); s2 = fmaf(x2, c0.z, s2); s2 = fmaf(x3, c0.w, s2);
        s2 = fmaf(x4, c1.x, s2); s2 = fmaf(x5, c1.y, s2); s2 = fmaf(x6, c1.z, s2); s2 = fmaf(x7, c1.w, s2);
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (lane == 0) {
        const float shift = s1 + b_shift[0];
        const float x = s2 + b_scale[0];
        const float scale = (x > 0.f ? x : expm1f(x)) + 1.0f;          // nn.ELU (alpha = 1) + 1
        *(float2*)(rowstats + row * 2) = make_float2(shift, scale);
    }
}

// ---- main kernel: class_sims_wide_kernel's contraction under a per-image table -------------------------------------------------------------
// A workgroup is (image b, group g of nw 32-row tiles of that image, query block qb of 32 queries): its table is image b's (or the shared bank's)
// queries 32 qb .. + 31, normalised HF's way while they are loaded into LDS -- row j by wave j % nw, lane-strided sum of squares + wave_sum, so a
// query's q^ depends on its Dt values alone, not on its position, its neighbours or the image.  Tiles never straddle images: wave w owns patches
// 32 (g nw + w) .. + 31 of image b; lanes past P (and waves past the image's last tile) compute on a clamped row and store nothing.  The
// contraction, the split of k over the lane halves and the row norm beside the MFMAs are class_sims_wide_kernel's.  Workgroups that share rows
// (they differ in qb only) are numbered onto ONE XCD, as there.
__global__ __launch_bounds__(512) void class_logits_kernel(const float* __restrict__ e, const float* __restrict__ queries,
                                                           const float* __restrict__ rowstats, const unsigned char* __restrict__ mask,
                                                           float* logits, float* scores, int P, int Q, int Dt, int nbanks, int nmasks,
                                                           int nqb, int groups, int tiles_img, int total_groups) {
    extern __shared__ __attribute__((aligned(16))) float lq[];
    const int ldq = Dt + 4;
    const int NT = blockDim.x, nw = NT >> 6;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int qb = slot % nqb, tg = (slot / nqb) * 8 + xcd;
    if (tg >= total_groups) return;                   // (whole workgroup: before any barrier)
    const int b = tg / groups, g = tg - b * groups;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5, l31 = lane & 31;
    float* lrow = lq + 32 * ldq;                      // [nw waves][3][32]: 1 / (|e| + eps), shift, scale of the wave's rows
    // ---- table: queries 32 qb .. + 31 of bank (nbanks == 1 ? 0 : b); rows past Q are zero
    const float* bank = queries + (int64_t)(nbanks == 1 ? 0 : b) * Q * Dt;
    const int q0 = qb * 32;
    for (int i = threadIdx.x; i < 32 * (Dt >> 2); i += NT) {
        const int j = i / (Dt >> 2), k4 = i - j * (Dt >> 2);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + j < Q) v = ((const float4*)(bank + (int64_t)(q0 + j) * Dt))[k4];
        *(float4*)(lq + j * ldq + k4 * 4) = v;
    }
    __syncthreads();
    for (int j = w; j < 32; j += nw) {                // HF: q / (|q| + 1e-6); an all-zero row stays all-zero
        float* qr = lq + j * ldq;
        float s = 0.f;
        for (int k = lane; k < Dt; k += 64) { const float v = qr[k]; s = s + v * v; }
        const float inv = 1.0f / (sqrtf(wave_sum(s)) + 1e-6f);
        for (int k = lane; k < Dt; k += 64) qr[k] = qr[k] * inv;
    }
    __syncthreads();
    // ---- the wave's rows
    int t = g * nw + w;
    const bool wave_on = t < tiles_img;
    if (!wave_on) t = tiles_img - 1;
    const int p0 = t * 32;
    const int p = min(p0 + l31, P - 1);
    const int64_t row = (int64_t)b * P + p;
    const float* er = e + row * Dt;
    const float* qr = lq + l31 * ldq;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    float ss = 0.f;
    const int nblk = 2 * ((Dt + 127) >> 7);
    auto kbase = [&](int blk, float& msk) {
        const int c0 = (blk >> 1) << 7;
        const bool act = (c0 + hi * 64) < Dt;          // a half-chunk past Dt (Dt % 128 == 64) feeds zeros: no divergence around MFMAs
        msk = act ? 1.f : 0.f;
        return (act ? c0 + hi * 64 : 0) + (blk & 1) * 32;
    };
    auto fetch = [&](int blk, float4 (&buf)[8]) {
        float m;
        const float* ptr = er + kbase(blk, m);
#pragma unroll
        for (int s = 0; s < 8; s++) buf[s] = *(const float4*)(ptr + s * 4);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto consume = [&](int blk, const float4 (&buf)[8]) {
        float msk;
        const float* q = qr + kbase(blk, msk);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            float4 a = buf[s];
            const float4 bq = *(const float4*)(q + s * 4);
            a.x *= msk; a.y *= msk; a.z *= msk; a.w *= msk;
            const float tq = ((a.x * a.x + a.y * a.y) + a.z * a.z) + a.w * a.w;          // separately rounded (contraction is off for this file)
            ss = ss + tq;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq.w, acc, 0, 0, 0);
        }
    };
    float4 bufA[8], bufB[8];
    fetch(0, bufA);
    for (int blk = 0; blk < nblk; blk += 2) {       // nblk is even
        fetch(blk + 1, bufB);
        consume(blk, bufA);
        fetch(min(blk + 2, nblk - 1), bufA);
        consume(blk + 1, bufB);
    }
    ss += __shfl_xor(ss, 32, 64);
    if (hi == 0) {
        const float2 st = *(const float2*)(rowstats + row * 2);
        lrow[(w * 3 + 0) * 32 + l31] = 1.0f / (sqrtf(ss) + 1e-6f);
        lrow[(w * 3 + 1) * 32 + l31] = st.x;
        lrow[(w * 3 + 2) * 32 + l31] = st.y;
    }
    __syncthreads();
    // ---- epilogue: acc[r] is row i = (r & 3) + 8 (r >> 2) + 4 hi of the tile, column l31 of the query block
    const int qcol = q0 + l31;
    const bool col_on = wave_on && qcol < Q;
    bool live = true;
    if (mask && qcol < Q) live = mask[(int64_t)(nmasks == 1 ? 0 : b) * Q + qcol] != 0;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float inv = lrow[(w * 3 + 0) * 32 + i], shift = lrow[(w * 3 + 1) * 32 + i], scale = lrow[(w * 3 + 2) * 32 + i];
        const float cosv = acc[r] * inv;
        const float lg = (cosv + shift) * scale;
        if (col_on && p0 + i < P) {
            const int64_t o = ((int64_t)b * P + p0 + i) * Q + qcol;
            logits[o] = live ? lg : -FLT_MAX;
            if (scores) scores[o] = live ? 1.0f / (1.0f + expf(-lg)) : 0.f;
        }
    }
}

static void class_logits_shape(int64_t P, int* nw, int* groups) {
    const int tiles = (int)((P + 31) / 32);
    *groups = (tiles + 7) / 8;                        // at most 8 waves per workgroup, evenly filled.  (Measured against a ceiling of 10 -- B/16 768^2 batch 32
                                                      // as 256 workgroups of 9 waves, one per CU: 30 queries 91 -> 76 us, but 1203 queries 1058 -> 1435 us:
                                                      // two 8-wave workgroups share a CU at Dt = 512 and hide each other's table load.  profiles/open_vocab.md)
    *nw = (tiles + *groups - 1) / *groups;
}

OWL_API int owl_class_logits_fwd(void* stream, const float* e, const float* queries, const void* feats_bf16, const float* w_shift, const float* b_shift,
                                 const float* w_scale, const float* b_scale, const unsigned char* mask, float* rowstats, float* logits, float* scores,
                                 int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t nmasks, int64_t Dt, int64_t D) {
    OWL_CHECK_ARG(e && queries && feats_bf16 && w_shift && b_shift && w_scale && b_scale && rowstats && logits, "owl_class_logits_fwd: null pointer");
    OWL_CHECK_ARG(B >= 1 && P >= 1 && P <= OV_MAX_PATCHES && B * P < ((int64_t)1 << 31),
                  "owl_class_logits_fwd: B >= 1, 1 <= P <= %d and B P < 2^31 required (B=%lld P=%lld)", OV_MAX_PATCHES, (long long)B, (long long)P);
    OWL_CHECK_ARG(Q >= 1 && Q <= OV_MAX_QUERIES, "owl_class_logits_fwd: 1 <= Q <= %d required (Q=%lld)", OV_MAX_QUERIES, (long long)Q);
    OWL_CHECK_ARG(Dt >= 64 && Dt % 64 == 0 && D >= 8 && D % 8 == 0, "owl_class_logits_fwd: Dt %% 64 == 0 and D %% 8 == 0 required (Dt=%lld D=%lld)",
                  (long long)Dt, (long long)D);
    OWL_CHECK_ARG(nbanks == 1 || nbanks == B, "owl_class_logits_fwd: queries is [nbanks, Q, Dt] with nbanks = B or 1 (got %lld for B=%lld)",
                  (long long)nbanks, (long long)B);
    OWL_CHECK_ARG(!mask || nmasks == 1 || nmasks == B, "owl_class_logits_fwd: mask is [nmasks, Q] with nmasks = B or 1 (got %lld for B=%lld)",
                  (long long)nmasks, (long long)B);
    OWL_CHECK_ARG((((uintptr_t)e | (uintptr_t)queries | (uintptr_t)feats_bf16 | (uintptr_t)w_shift | (uintptr_t)w_scale) & 15) == 0 && ((uintptr_t)rowstats & 7) == 0,
                  "owl_class_logits_fwd: e, queries, feats, w_shift and w_scale must be 16-byte aligned, rowstats 8-byte aligned");
    int nw, groups;
    class_logits_shape(P, &nw, &groups);
    const size_t shmem = (size_t)(32 * (Dt + 4) + 96 * nw) * sizeof(float);
    OWL_CHECK_ARG(shmem <= 160 * 1024, "owl_class_logits_fwd: Dt=%lld too large for the LDS-resident query table", (long long)Dt);
    static unsigned long long attr_done = 0;
    OWL_ONCE_PER_DEVICE(attr_done, (void)hipFuncSetAttribute((const void*)class_logits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int nqb = (int)((Q + 31) / 32);
    const int64_t total_groups = B * groups;
    OWL_CHECK_ARG((total_groups + 7) / 8 * nqb * 8 < ((int64_t)1 << 31), "owl_class_logits_fwd: B, P and Q together give too many workgroups for one launch");
    const int64_t rows = B * P;
    hipLaunchKernelGGL(logit_rowstats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)feats_bf16, w_shift, w_scale,
                       b_shift, b_scale, rowstats, rows, (int)D);
    OWL_LAUNCH_CHECK();
    const int64_t grid = (total_groups + 7) / 8 * nqb * 8;
    hipLaunchKernelGGL(class_logits_kernel, dim3((unsigned)grid), dim3(64 * nw), shmem, (hipStream_t)stream, e, queries, rowstats, mask, logits, scores,
                       (int)P, (int)Q, (int)Dt, (int)nbanks, (int)nmasks, nqb, groups, (int)((P + 31) / 32), (int)total_groups);
    OWL_LAUNCH_CHECK();
    return 0;
}
