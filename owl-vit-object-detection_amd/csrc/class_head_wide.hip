// Class head for label sets beyond 10 classes (3C > 32 prompts: more than the one 32-column MFMA tile of heads.hip / backward.hip), forward and
// backward.  A file of its own: the narrow kernels' translation units -- and with them their code and their bits -- stay as they are.
#include "common.h"

// ---- wide class head: label sets beyond 10 classes (3C > 32) -------------------------------------------
// The query bank is cut into blocks of 10 classes = 30 prompts.  qhat is laid out [nblk][32][Dt] with nblk = ceil(C / 10): class c sits in
// block c / 10, its three prompts in rows 3 (c % 10) .. + 2, rows 30 and 31 of every block (and the rows of classes >= C) are zero.  Every
// 32-column MFMA tile then holds whole prompt triples and the max-of-3 never straddles a tile.  One block of the wide layout is exactly the
// [32][Dt] table the narrow kernels take for those <= 10 classes.
__global__ __launch_bounds__(64) void qhat_wide_kernel(const float* __restrict__ q, float* qhat, float* qnorm, int nq, int Dt) {
    const int jw = blockIdx.x, lane = threadIdx.x;            // row of the wide layout
    const int b = jw >> 5, r = jw & 31;
    const int j = 30 * b + r;                                  // row of the [3C][Dt] bank
    if (r >= 30 || j >= nq) {
        for (int k = lane; k < Dt; k += 64) qhat[(int64_t)jw * Dt + k] = 0.f;
        if (lane == 0 && qnorm) qnorm[jw] = 0.f;
        return;
    }
    // (the arithmetic of qhat_kernel, in its order: a block's rows carry the bits a 10-class call gives them)
    float s = 0.f;
    for (int k = lane; k < Dt; k += 64) { const float v = q[(int64_t)j * Dt + k]; s += v * v; }
    const float n = sqrtf(wave_sum(s));
    if (lane == 0 && qnorm) qnorm[jw] = n;
    for (int k = lane; k < Dt; k += 64) qhat[(int64_t)jw * Dt + k] = q[(int64_t)j * Dt + k] / n + 1e-6f;
}

OWL_API int owl_query_normalize_wide(void* stream, const float* queries, float* qhat_wide, float* qnorm, int64_t nq, int64_t Dt) {
    OWL_CHECK_ARG(queries && qhat_wide, "owl_query_normalize_wide: null pointer");
    OWL_CHECK_ARG(nq >= 3 && nq % 3 == 0 && nq <= 3 * OWL_WIDE_MAX_CLASSES, "owl_query_normalize_wide: need queries = 3 C with 1 <= C <= %d (got %lld)",
                  OWL_WIDE_MAX_CLASSES, (long long)nq);
    OWL_CHECK_ARG(Dt >= 1, "owl_query_normalize_wide: Dt >= 1 required");
    const int nblk = (int)((nq / 3 + 9) / 10);
    hipLaunchKernelGGL(qhat_wide_kernel, dim3(32 * nblk), dim3(64), 0, (hipStream_t)stream, queries, qhat_wide, qnorm, (int)nq, (int)Dt);
    OWL_LAUNCH_CHECK();
    return 0;
}

// class_sims_kernel for one query block per workgroup: the block's [32][Dt+4] table in LDS, the same split of the contraction over lanes (hi = 0 / 1
// take the two 64-wide halves of each 128-chunk), the same order of the products and of the row norm's sums -- column c of the result carries the bits
// the narrow kernel gives for a 10-class call on classes 10 (c / 10) .. + 9 (tests/test_labelsets_gpu.py holds it to that).  The workgroups that share
// a row tile differ in the query block only; they are numbered so that they run on ONE XCD one after the other (consecutive workgroup ids go round
// the 8 XCDs): the row tile's e is then read from HBM once and from that XCD's L2 by the other blocks.  inv_norm is written by block 0.
__global__ __launch_bounds__(640) void class_sims_wide_kernel(const float* __restrict__ e, const float* __restrict__ qhat_wide,
                                                              float* sims, unsigned char* argmax, float* inv_norm,
                                                              int64_t rows, int Dt, int C, int nqb, int row_tiles) {
    extern __shared__ __attribute__((aligned(16))) float lq[];
    const int ldq = Dt + 4;
    const int NT = blockDim.x, nw = NT >> 6;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int qb = slot % nqb, tile = (slot / nqb) * 8 + xcd;
    if (tile >= row_tiles) return;                    // (whole workgroup: before any barrier)
    const float* qhat = qhat_wide + (int64_t)qb * 32 * Dt;
    const int Cb = min(10, C - 10 * qb);              // classes of this block
    float* lnorm = lq + 32 * ldq;   // [nw waves][32]
    for (int i = threadIdx.x; i < 32 * (Dt >> 2); i += NT) {
        const int j = i / (Dt >> 2), k4 = i - j * (Dt >> 2);
        *(float4*)(lq + j * ldq + k4 * 4) = ((const float4*)(qhat + (int64_t)j * Dt))[k4];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 5;
    const int64_t r0 = ((int64_t)tile * nw + w) * 32;
    int64_t row = r0 + (lane & 31);
    const bool valid = row < rows;
    if (!valid) row = rows - 1;
    const float* er = e + row * Dt;
    const float* qr = lq + (lane & 31) * ldq;
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
        const float* p = er + kbase(blk, m);
#pragma unroll
        for (int s = 0; s < 8; s++) buf[s] = *(const float4*)(p + s * 4);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto consume = [&](int blk, const float4 (&buf)[8]) {
        float msk;
        const float* q = qr + kbase(blk, msk);
#pragma unroll
        for (int s = 0; s < 8; s++) {
            float4 a = buf[s];
            const float4 b = *(const float4*)(q + s * 4);
            a.x *= msk; a.y *= msk; a.z *= msk; a.w *= msk;
            {
                // separately rounded products and sums, in class_sims_kernel's order (its bits)
#pragma clang fp contract(off)
                const float t = ((a.x * a.x + a.y * a.y) + a.z * a.z) + a.w * a.w;
                ss = ss + t;
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
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
    const float inv = 1.0f / (sqrtf(ss) + 1e-6f);
    if (hi == 0) {
        lnorm[w * 32 + lane] = inv;
        if (valid && inv_norm && qb == 0) inv_norm[row] = inv;
    }
    __syncthreads();
    const int j = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float v0 = acc[r] * lnorm[w * 32 + i];
        const float v1 = __shfl_down(v0, 1, 64), v2 = __shfl_down(v0, 2, 64);
        float best = v0; int arg = 0;
        if (v1 > best) { best = v1; arg = 1; }
        if (v2 > best) { best = v2; arg = 2; }
        const int64_t orow = r0 + i;
        if (j % 3 == 0 && j / 3 < Cb && orow < rows) {
            sims[orow * C + 10 * qb + j / 3] = best;
            if (argmax) argmax[orow * C + 10 * qb + j / 3] = (unsigned char)arg;
        }
    }
}

// waves per workgroup: class_sims_waves() of heads.hip (one workgroup of <= 10 waves per CU and query block)
static int wide_sims_waves(int64_t rows) {
    const int64_t total = (rows + 31) / 32;
    const int64_t w = (total + 255) / 256;
    return (int)(w < 4 ? 4 : (w > 10 ? 10 : w));
}

OWL_API int owl_class_sims_wide_fwd(void* stream, const float* e, const float* qhat_wide, float* sims, unsigned char* argmax,
                                       float* inv_norm, int64_t rows, int64_t Dt, int64_t C) {
    OWL_CHECK_ARG(e && qhat_wide && sims, "owl_class_sims_wide_fwd: null pointer");
    OWL_CHECK_ARG(rows >= 1 && rows < ((int64_t)1 << 31), "owl_class_sims_wide_fwd: 1 <= rows < 2^31 required");
    OWL_CHECK_ARG(Dt % 64 == 0 && Dt >= 64 && C >= 1 && C <= OWL_WIDE_MAX_CLASSES, "owl_class_sims_wide_fwd: Dt %% 64 == 0 and 1 <= C <= %d required (Dt=%lld C=%lld)",
                  OWL_WIDE_MAX_CLASSES, (long long)Dt, (long long)C);
    const int nw = wide_sims_waves(rows);
    const size_t shmem = (size_t)(32 * (Dt + 4) + 32 * nw) * sizeof(float);
    OWL_CHECK_ARG(shmem <= 160 * 1024, "owl_class_sims_wide_fwd: Dt=%lld too large for the LDS-resident query table", (long long)Dt);
    static unsigned long long attr_done = 0;
    OWL_ONCE_PER_DEVICE(attr_done, (void)hipFuncSetAttribute((const void*)class_sims_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int64_t total = (rows + 31) / 32;
    const int row_tiles = (int)((total + nw - 1) / nw), nqb = (int)((C + 9) / 10);
    const int64_t grid = (int64_t)((row_tiles + 7) / 8) * nqb * 8;
    hipLaunchKernelGGL(class_sims_wide_kernel, dim3((unsigned)grid), dim3(64 * nw), shmem, (hipStream_t)stream, e, qhat_wide, sims, argmax, inv_norm,
                       rows, (int)Dt, (int)C, nqb, row_tiles);
    OWL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// wide class head backward (label sets beyond 10 classes; the [nblk][32][Dt] query layout above).  One class per lane and a gathered
// LDS-resident bank do not survive C > 64 or a bank of Q Dt 4 bytes, so de is a dense product on the exact-f32 matrix core:
//   de = inv * (A . qhat_wide) - coef_e * e,   A[r, j] = dsims[r, c] * [j = 32 (c / 10) + 3 (c % 10) + argmax]   (f32, [rows, Qw] x [Qw, Dt])
// rounded once to bf16, coef_e formed as in class_sims_bwd_kernel.  A workgroup of four waves owns 32 rows: it routes the rows' upstream into an
// LDS tile of 256 wide-layout columns at a time (= 80 classes), writes that tile -- scaled by inv, as bf16 -- to G[rows, Qp] (Qp = Qw rounded up
// to 256: dqhat = G^T e then goes through the TN kernel like every other dW; the pad columns are written as zeros), and feeds it to the MFMAs as
// the A operand; the B operand (qhat rows) comes from the L2.  Wave w owns the 32-column tiles w, w + 4, ... of Dt.  Fixed summation order, no
// atomics: two runs give equal bits.
// ---------------------------------------------------------------------------------------------------
#define WB_LD 260          // row stride (words) of the routed-upstream tile: 16-byte aligned rows
template <int NT>
__global__ __launch_bounds__(256) void class_sims_wide_bwd_kernel(const float* __restrict__ dsims, const float* __restrict__ sims,
                                                                  const unsigned char* __restrict__ argmax, const float* __restrict__ inv_norm,
                                                                  const float* __restrict__ e, const float* __restrict__ qhat, bf16_t* de,
                                                                  bf16_t* G, bf16_t* e_bf16, int64_t rows, int Dt, int C, int Qw, int Qp) {
    __shared__ __attribute__((aligned(16))) float ga[32 * WB_LD];
    __shared__ float s_inv[32], s_coef[32];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const int nrows = (int)min((int64_t)32, rows - r0);
    for (int i = w; i < 32; i += 4) {                   // per-row scalars: 1 / norm and the coefficient of e
        float gs = 0.f, inv = 0.f;
        if (i < nrows) {
            const int64_t r = r0 + i;
            inv = inv_norm[r];
            for (int c = lane; c < C; c += 64) gs += dsims[r * C + c] * sims[r * C + c];
        }
        gs = wave_sum(gs);
        if (lane == 0) {
            const float nrm = 1.0f / inv - 1e-6f;
            s_inv[i] = inv;
            s_coef[i] = (i < nrows && nrm > 0.f) ? gs * inv / nrm : 0.f;    // (an all-zero row: nrm = 0 exactly; class_sims_bwd_kernel's select)
        }
    }
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    for (int q0 = 0; q0 < Qp; q0 += 256) {
        __syncthreads();                                // the MFMAs of the previous chunk have read the tile
        for (int i = tid; i < 32 * WB_LD; i += 256) ga[i] = 0.f;
        __syncthreads();
        const int c0 = (q0 >> 5) * 10, nc = min(80, C - c0);
        for (int idx = tid; idx < 32 * 80; idx += 256) {
            const int i = idx / 80, cl = idx - i * 80;
            if (i < nrows && cl < nc) {
                const int64_t o = (r0 + i) * C + c0 + cl;
                const int am = min((int)argmax[o], 2);
                ga[i * WB_LD + (cl / 10) * 32 + 3 * (cl % 10) + am] = dsims[o];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < 32 * 128; idx += 256) {
            const int i = idx >> 7, p = idx & 127;
            if (i < nrows) {
                const float inv = s_inv[i];
                const float2 v = *(const float2*)(ga + i * WB_LD + 2 * p);
                ((unsigned*)(G + (r0 + i) * Qp + q0))[p] = pack_bf2(v.x * inv, v.y * inv);
            }
        }
        const int kmax = min(256, Qw - q0);             // (the pad chunk beyond Qw has no qhat rows: nothing to multiply)
        for (int k8 = 0; k8 < kmax; k8 += 8) {
            // lanes hi = 0 / 1 take k8 .. k8 + 3 / k8 + 4 .. k8 + 7: one 16-byte LDS read feeds four MFMAs per column tile
            const int k = k8 + 4 * hi;
            const float4 a = *(const float4*)(ga + l31 * WB_LD + k);
            const float* qb = qhat + (int64_t)(q0 + k) * Dt + l31;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const int n0 = (w + 4 * t) * 32;
                if (n0 < Dt) {                          // wave-uniform
                    const float b0 = qb[n0], b1 = qb[Dt + n0], b2 = qb[2 * Dt + n0], b3 = qb[3 * Dt + n0];
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b2, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b3, acc[t], 0, 0, 0);
                }
            }
        }
    }
    // acc[t][r]: row i = (r & 3) + 8 (r >> 2) + 4 hi, column (w + 4 t) 32 + lane % 32
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n0 = (w + 4 * t) * 32;
        if (n0 >= Dt) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (i < nrows) {
                const int64_t o = (r0 + i) * Dt + n0 + l31;
                const float ev = e[o];
                de[o] = f2bf(s_inv[i] * acc[t][r] - s_coef[i] * ev);
                e_bf16[o] = f2bf(ev);
            }
        }
    }
}

// dQ from dqhat in the wide layout: bank row j = 30 b + r reads dqhat row 32 b + r (qhat_bwd_kernel's arithmetic)
__global__ __launch_bounds__(64) void qhat_wide_bwd_kernel(const float* __restrict__ dqhat, const float* __restrict__ q, float* dq, int Dt) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const float* dh = dqhat + (int64_t)(32 * (j / 30) + j % 30) * Dt;
    float ss = 0.f, dt = 0.f;
    for (int k = lane; k < Dt; k += 64) { const float v = q[(int64_t)j * Dt + k]; ss += v * v; dt += v * dh[k]; }
    ss = wave_sum(ss); dt = wave_sum(dt);
    const float n = sqrtf(ss);
    for (int k = lane; k < Dt; k += 64) {
        const float qn = q[(int64_t)j * Dt + k] / n;
        dq[(int64_t)j * Dt + k] += (dh[k] - (dt / n) * qn) / n;
    }
}

OWL_API int owl_class_sims_wide_bwd(void* stream, const float* dsims, const float* sims, const unsigned char* argmax, const float* inv_norm,
                                       const float* e, const float* qhat_wide, void* de_bf16, void* g_bf16, void* e_bf16, int64_t rows,
                                       int64_t Dt, int64_t C, int64_t Qp) {
    OWL_CHECK_ARG(dsims && sims && argmax && inv_norm && e && qhat_wide && de_bf16 && g_bf16 && e_bf16, "owl_class_sims_wide_bwd: null pointer");
    OWL_CHECK_ARG(rows >= 1 && C >= 1 && C <= OWL_WIDE_MAX_CLASSES, "owl_class_sims_wide_bwd: rows >= 1 and 1 <= C <= %d required (C=%lld)", OWL_WIDE_MAX_CLASSES, (long long)C);
    OWL_CHECK_ARG(Dt % 32 == 0 && Dt >= 32 && Dt <= 1024, "owl_class_sims_wide_bwd: Dt %% 32 == 0 and Dt <= 1024 required (Dt=%lld)", (long long)Dt);
    const int Qw = 32 * (int)((C + 9) / 10);
    OWL_CHECK_ARG(Qp == (Qw + 255) / 256 * 256, "owl_class_sims_wide_bwd: G is [rows, Qp] with Qp = 32 ceil(C / 10) rounded up to 256 (= %d, got %lld)",
                  (Qw + 255) / 256 * 256, (long long)Qp);
    const dim3 grid((unsigned)((rows + 31) / 32));
    const int per_wave = (int)((Dt / 32 + 3) / 4);
#define OWL_WIDE_BWD(NT_)                                                                                                                    \
    hipLaunchKernelGGL(class_sims_wide_bwd_kernel<NT_>, grid, dim3(256), 0, (hipStream_t)stream, dsims, sims, argmax, inv_norm, e, qhat_wide, \
                       (bf16_t*)de_bf16, (bf16_t*)g_bf16, (bf16_t*)e_bf16, rows, (int)Dt, (int)C, Qw, (int)Qp)
    if (per_wave <= 1) OWL_WIDE_BWD(1);
    else if (per_wave <= 2) OWL_WIDE_BWD(2);
    else if (per_wave <= 4) OWL_WIDE_BWD(4);
    else if (per_wave <= 6) OWL_WIDE_BWD(6);
    else OWL_WIDE_BWD(8);
#undef OWL_WIDE_BWD
    OWL_LAUNCH_CHECK();
    return 0;
}

// dqueries[3C, Dt] += d(qhat -> Q) of dqhat (f32, wide layout [>= 32 ceil(C / 10), Dt])
OWL_API int owl_query_normalize_wide_bwd(void* stream, const float* dqhat_wide, const float* queries, float* dqueries, int64_t nq, int64_t Dt) {
    OWL_CHECK_ARG(dqhat_wide && queries && dqueries, "owl_query_normalize_wide_bwd: null pointer");
    OWL_CHECK_ARG(nq >= 3 && nq % 3 == 0 && nq <= 3 * OWL_WIDE_MAX_CLASSES && Dt >= 1, "owl_query_normalize_wide_bwd: need queries = 3 C with 1 <= C <= %d (got %lld)",
                  OWL_WIDE_MAX_CLASSES, (long long)nq);
    hipLaunchKernelGGL(qhat_wide_bwd_kernel, dim3((unsigned)nq), dim3(64), 0, (hipStream_t)stream, dqhat_wide, queries, dqueries, (int)Dt);
    OWL_LAUNCH_CHECK();
    return 0;
}

