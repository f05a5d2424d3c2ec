// Open-vocabulary class head, backward: the adjoint of owl_class_logits_fwd (open_vocab.hip, whose translation unit and bits stay as they are).
//   logit[b, p, q] = (e^_p . q^_{b,q} + shift_p) * scale_p,   e^ = e / (|e| + 1e-6),  q^ = Q / (|Q| + 1e-6),  scale = elu(s) + 1
// With the upstream g = dlogits SELECTED to 0 where mask[b, q] == 0 (never multiplied: Inf / NaN there changes nothing), per row r of image b:
//   T_r    = sum_q g[r, q] q^_q                       (exact-f32 MFMA product, [32 rows, Q] x [Q, Dt]; d(e^) = scale_r T_r)
//   gs_r   = sum_q g[r, q],   c_r = e^_r . T_r  = sum_q g cos          (the cosine term is never recovered as logit / scale)
//   dshift = scale gs,  dscale = c + shift gs,  ds = dscale (scale > 1 ? 1 : scale)          (ELU' read from the saved scale)
//   dfeats_r = dshift w_shift + ds w_scale            (f32, plain store)
//   de_r   = inv_r scale_r (T_r - e_r c_r / |e_r|)    (bf16; the second term is 0 for an all-zero row: de = d(e^) / 1e-6, never NaN)
//   dq^_{b,q} = sum_{r in image b} g[r, q] (inv_r scale_r) e_r         (exact-f32 MFMA product per row chunk, partial slabs added in index order)
//   dq     = (dq^ - u (q^ . dq^)) / (|q| + 1e-6),  u = q / |q| (0 for an all-zero row)
// Compiled with contraction off (csrc/build.sh): every written operation rounds once, the count tests/open_vocab_bwd_reference.py bounds.  No atomics,
// nothing allocated, no host sync; every sum has one fixed order that depends on (P, Q, Dt) alone, not on the batch: two runs give equal bits and an
// image's block carries the same bits wherever it stands.
//
// Gradients of the head's own four tensors (owl_class_logits_bwd_head): the row pass also stores its (dshift_r, ds_r) into `rowgrad`, then
//   dW_shift[c] = sum_r dshift_r feats[r, c]   db_shift = sum_r dshift_r   dW_scale[c] = sum_r ds_r feats[r, c]   db_scale = sum_r ds_r     (r over all B P rows)
// in two launches (ovb_head_part_kernel, ovb_head_finish_kernel).  Accumulation is FLOAT64, one rounding to f32 at the final store: a bf16 feature times
// an f32 row scalar is exact in f64 (8 x 24 significand bits), so the only roundings of the reduction are its f64 adds (2^-53 each) and the last
// conversion.  The reason: the sum runs over B P rows (73 728 at B/16, batch 32) of terms that cancel, so an f32 chain's error would grow with the batch
// and stand beside -- not under -- what dshift / ds inherit from the row pass; in f64 the bound is the inherited one plus half an f32 ulp at every batch
// size.  It costs nothing: the pass is bound by the one read of feats, and gfx950's vector f64 adds run at half the f32 rate.
#include "common.h"

#define OVB_MAX_QUERIES 4096
#define OVB_MAX_PATCHES 8192
#define OVB_LD 260          // row stride (words) of the upstream tile: 16-byte aligned rows

// ---- q^ = q / (|q| + 1e-6), |q| and 1 / (|q| + 1e-6) of every query; one wave per row of the [nbanks][Qp][Dt] table, rows Q .. Qp - 1 zero ----------
// (class_logits_kernel's arithmetic: lane-strided sum of squares, wave_sum, one reciprocal, one multiply per element)
__global__ __launch_bounds__(64) void ovb_qhat_kernel(const float* __restrict__ queries, float* qhat, float* qnrm, float* qinv, int Q, int Qp, int Dt) {
    const int lane = threadIdx.x;
    const int bank = blockIdx.x / Qp, j = blockIdx.x - bank * Qp;
    float* out = qhat + (int64_t)blockIdx.x * Dt;
    if (j >= Q) {
        for (int k = lane; k < Dt; k += 64) out[k] = 0.f;
        if (lane == 0) { qnrm[blockIdx.x] = 0.f; qinv[blockIdx.x] = 0.f; }
        return;
    }
    const float* q = queries + ((int64_t)bank * Q + j) * Dt;
    float s = 0.f;
    for (int k = lane; k < Dt; k += 64) { const float v = q[k]; s = s + v * v; }
    const float n = sqrtf(wave_sum(s));
    const float inv = 1.0f / (n + 1e-6f);
    for (int k = lane; k < Dt; k += 64) out[k] = q[k] * inv;
    if (lane == 0) { qnrm[blockIdx.x] = n; qinv[blockIdx.x] = inv; }
}

// ---- row pass: de, dfeats and the row factor inv scale of 32 rows of ONE image -----------------------------------------------------------------
// class_sims_wide_bwd_kernel's shape: four waves, the rows' selected upstream in an LDS tile of 256 queries at a time as the MFMAs' A operand, q^ rows
// from the L2 as the B operand, wave w owns the 32-column tiles w, w + 4, ... of Dt.  The row norm and e . T are summed from the accumulator
// registers: over the wave's tiles in a lane, over the 32 lanes of a half by five xor steps, over the four waves in index order.
template <int NT>
__global__ __launch_bounds__(256) void ovb_rows_kernel(const float* __restrict__ dlogits, const float* __restrict__ e, const float* __restrict__ qhat,
                                                       const float* __restrict__ rowstats, const unsigned char* __restrict__ mask,
                                                       const float* __restrict__ w_shift, const float* __restrict__ w_scale, bf16_t* de, float* dfeats,
                                                       float* rowfac, float* rowgrad, int P, int Q, int Qp, int Dt, int D, int nbanks, int nmasks,
                                                       int tiles_img) {
    __shared__ __attribute__((aligned(16))) float ga[32 * OVB_LD];
    __shared__ float s_gs[32], s_part[2][4][32], s_a[32], s_coef[32], s_dsh[32], s_ds[32];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.x / tiles_img, p0 = (blockIdx.x - b * tiles_img) * 32;
    const int nrows = min(32, P - p0);
    const int64_t r0 = (int64_t)b * P + p0;
    const unsigned char* mrow = mask ? mask + (int64_t)(nmasks == 1 ? 0 : b) * Q : nullptr;
    const float* bank = qhat + (int64_t)(nbanks == 1 ? 0 : b) * Qp * Dt;
    for (int i = w; i < 32; i += 4) {                   // gs: lane-strided over the queries, then the butterfly
        float gs = 0.f;
        if (i < nrows)
            for (int c = lane; c < Q; c += 64) {
                const bool live = !mrow || mrow[c] != 0;
                float v = 0.f;
                if (live) v = dlogits[(r0 + i) * Q + c];
                gs = gs + v;
            }
        gs = wave_sum(gs);
        if (lane == 0) s_gs[i] = gs;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    for (int q0 = 0; q0 < Qp; q0 += 256) {
        __syncthreads();                                // the MFMAs of the previous chunk have read the tile
        {
            const int q = q0 + tid;                     // one column of the tile per thread
            const bool live = q < Q && (!mrow || mrow[q] != 0);
            for (int i = 0; i < 32; i++) {
                float v = 0.f;
                if (live && i < nrows) v = dlogits[(r0 + i) * Q + q];
                ga[i * OVB_LD + tid] = v;
            }
        }
        __syncthreads();
        const int kmax = min(256, Qp - q0);             // a multiple of 32
        for (int k8 = 0; k8 < kmax; k8 += 8) {
            const int k = k8 + 4 * hi;                  // lanes hi = 0 / 1 take k8 .. k8 + 3 / k8 + 4 .. k8 + 7
            const float4 a = *(const float4*)(ga + l31 * OVB_LD + k);
            const float* qb = bank + (int64_t)(q0 + k) * Dt + l31;
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
    // acc[t][r]: row i = (r & 3) + 8 (r >> 2) + 4 hi, column (w + 4 t) 32 + l31.  Rows past the image's last compute on its last row and store nothing.
    float pss[16], pet[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { pss[r] = 0.f; pet[r] = 0.f; }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n0 = (w + 4 * t) * 32;
        if (n0 < Dt) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = min((r & 3) + 8 * (r >> 2) + 4 * hi, nrows - 1);
                const float ev = e[(r0 + i) * Dt + n0 + l31];
                pss[r] = pss[r] + ev * ev;
                pet[r] = pet[r] + ev * acc[t][r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            pss[r] = pss[r] + __shfl_xor(pss[r], o, 64);
            pet[r] = pet[r] + __shfl_xor(pet[r], o, 64);
        }
        if (l31 == 0) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;
            s_part[0][w][i] = pss[r];
            s_part[1][w][i] = pet[r];
        }
    }
    __syncthreads();
    if (tid < 32) {
        const int i = tid;
        const float ss = ((s_part[0][0][i] + s_part[0][1][i]) + s_part[0][2][i]) + s_part[0][3][i];
        const float et = ((s_part[1][0][i] + s_part[1][1][i]) + s_part[1][2][i]) + s_part[1][3][i];
        const int64_t row = r0 + min(i, nrows - 1);
        const float2 st = *(const float2*)(rowstats + row * 2);
        const float shift = st.x, scale = st.y;
        const float nrm = sqrtf(ss);
        const float inv = 1.0f / (nrm + 1e-6f);
        const float c = inv * et;                       // sum_q g cos
        const float gs = s_gs[i];
        const float dshift = scale * gs;
        const float dscale = c + shift * gs;
        const float ds = dscale * (scale > 1.0f ? 1.0f : scale);
        const float a = inv * scale;
        s_a[i] = a;
        s_coef[i] = nrm > 0.f ? c / nrm : 0.f;          // (an all-zero row: torch's gradient of the norm at 0)
        s_dsh[i] = dshift;
        s_ds[i] = ds;
        if (i < nrows) rowfac[row] = a;
        if (rowgrad && i < nrows) *(float2*)(rowgrad + row * 2) = make_float2(dshift, ds);          // (the head's own gradients: ovb_head_part_kernel)
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n0 = (w + 4 * t) * 32;
        if (n0 >= Dt) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (i < nrows) {
                const int64_t o = (r0 + i) * Dt + n0 + l31;
                const float ce = s_coef[i] * e[o];
                const float inner = acc[t][r] - ce;
                de[o] = f2bf(s_a[i] * inner);
            }
        }
    }
    if (dfeats) {
        const int d4 = D >> 2;
        for (int idx = tid; idx < nrows * d4; idx += 256) {
            const int i = idx / d4, c4 = idx - i * d4;
            const float4 ws = *(const float4*)(w_shift + c4 * 4), wc = *(const float4*)(w_scale + c4 * 4);
            const float dsh = s_dsh[i], ds = s_ds[i];
            float4 o;
            o.x = dsh * ws.x + ds * wc.x; o.y = dsh * ws.y + ds * wc.y; o.z = dsh * ws.z + ds * wc.z; o.w = dsh * ws.w + ds * wc.w;
            *(float4*)(dfeats + (r0 + i) * D + c4 * 4) = o;
        }
    }
}

// ---- dq^ partial slabs: part[b][s][32 qb + i][k] = sum over rows p of chunk s of image b of g[p, q] rowfac_p e[p, k] ----------------------------------
// A workgroup is (query block, row chunk, image); the MFMA's A operand is the selected upstream times the row factor (one row per lane half and
// instruction, rows in ascending order), its B operand the rows of e; wave w owns the 32-column tiles w, w + 4, ... of Dt.
template <int NT>
__global__ __launch_bounds__(256) void ovb_dq_kernel(const float* __restrict__ dlogits, const float* __restrict__ e, const float* __restrict__ rowfac,
                                                     const unsigned char* __restrict__ mask, float* part, int P, int Q, int Qp, int Dt, int nmasks,
                                                     int nqb, int S, int chunk) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int qb = blockIdx.x % nqb, s = (blockIdx.x / nqb) % S, b = blockIdx.x / (nqb * S);
    if (w * 32 >= Dt) return;                           // (whole wave; no barrier in this kernel)
    const int q = qb * 32 + l31;
    bool colok = q < Q;
    if (colok && mask) colok = mask[(int64_t)(nmasks == 1 ? 0 : b) * Q + q] != 0;
    const int pbeg = s * chunk, pend = min(P, pbeg + chunk);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    for (int pp = pbeg; pp < pend; pp += 8) {           // chunk is a multiple of 8
        float a[4];
        const float* er[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = pp + 2 * j + hi;
            const int64_t row = (int64_t)b * P + min(p, P - 1);
            a[j] = 0.f;
            if (colok && p < pend) a[j] = dlogits[row * Q + q] * rowfac[row];
            er[j] = e + row * Dt + l31;
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int n0 = (w + 4 * t) * 32;
            if (n0 < Dt) {                              // wave-uniform
#pragma unroll
                for (int j = 0; j < 4; j++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], er[j][n0], acc[t], 0, 0, 0);
            }
        }
    }
    float* out = part + ((int64_t)(b * S + s) * Qp + qb * 32) * Dt;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n0 = (w + 4 * t) * 32;
        if (n0 >= Dt) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * hi;
            out[(int64_t)i * Dt + n0 + l31] = acc[t][r];
        }
    }
}

// ---- dq^ = the partial slabs added in index order (a bank per image: the image's S chunks; a shared bank: every image's, image-major), then dq^ -> dq.
// One wave per query; lane l holds columns l, l + 64, ... (Dt <= 1024: 16 of them).
__global__ __launch_bounds__(64) void ovb_dq_finish_kernel(const float* __restrict__ part, const float* __restrict__ queries, const float* __restrict__ qhat,
                                                           const float* __restrict__ qnrm, const float* __restrict__ qinv, float* dqueries, int Q, int Qp,
                                                           int Dt, int first_per_bank, int nparts) {
    const int lane = threadIdx.x;
    const int bank = blockIdx.x / Q, j = blockIdx.x - bank * Q;
    const float* p0 = part + ((int64_t)bank * first_per_bank * Qp + j) * Dt;
    const float* qh = qhat + ((int64_t)bank * Qp + j) * Dt;
    float v[16];
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 16; c++) {
        const int k = lane + 64 * c;
        v[c] = 0.f;
        if (k < Dt) {
            float s = 0.f;
            for (int i = 0; i < nparts; i++) s = s + p0[(int64_t)i * Qp * Dt + k];
            v[c] = s;
            dot = dot + qh[k] * s;
        }
    }
    dot = wave_sum(dot);
    const float n = qnrm[bank * Qp + j], inv = qinv[bank * Qp + j];
    const float* q = queries + ((int64_t)bank * Q + j) * Dt;
    float* out = dqueries + ((int64_t)bank * Q + j) * Dt;
#pragma unroll
    for (int c = 0; c < 16; c++) {
        const int k = lane + 64 * c;
        if (k < Dt) {
            const float u = n > 0.f ? q[k] / n : 0.f;
            const float ud = u * dot;
            out[k] = (v[c] - ud) * inv;
        }
    }
}

// ---- gradients of logit_shift / logit_scale: partial sums of one (image, chunk of OVB_HEAD_CHUNK rows, block of 128 columns) ------------------------
// 256 threads = 16 row lanes x 16 column lanes; a thread owns 8 adjacent columns (one 16-byte load of bf16 features per row) and the rows
// pbeg + rl, pbeg + rl + 16, ... of the chunk in ascending order.  A row of the block is 256 contiguous bytes, a wave reads four rows at once: at
// D = 128 every lane of every wave has columns (a lane-per-8-columns layout ALONG the row would leave 48 lanes of a wave idle there).  The 16 row
// lanes are then added in index order through LDS (the shift sums, then the scale sums, through one tile); column lane 0 also sums the two row scalars themselves (the bias gradients; block 0 stores them).
// part[(b S + s)][2 D + 2] f64, laid out w_shift | w_scale | b_shift | b_scale.  The chunking is a constant: a function of nothing but the source.
#define OVB_HEAD_CHUNK 256
__global__ __launch_bounds__(256) void ovb_head_part_kernel(const bf16_t* __restrict__ feats, const float* __restrict__ rowgrad, double* part, int P, int D,
                                                            int S, int ncb) {
    __shared__ double s_acc[16][16][9];                 // [row lane][column lane][8 sums (+1: bank spread)]: the shift sums, then the scale sums
    __shared__ double s_b[16][2];
    const int tid = threadIdx.x, cl = tid & 15, rl = tid >> 4;
    const int cb = blockIdx.x % ncb, s = (blockIdx.x / ncb) % S, b = blockIdx.x / (ncb * S);
    const int pbeg = s * OVB_HEAD_CHUNK, pend = min(P, pbeg + OVB_HEAD_CHUNK);
    const int c0 = cb * 128 + cl * 8;
    const bool colok = c0 < D;                          // (D % 8 == 0: a thread's eight columns exist together)
    double ash[8], asc[8], bsh = 0.0, bsc = 0.0;
#pragma unroll
    for (int j = 0; j < 8; j++) { ash[j] = 0.0; asc[j] = 0.0; }
    if (colok) {
#pragma unroll 4
        for (int p = pbeg + rl; p < pend; p += 16) {
            const int64_t row = (int64_t)b * P + p;
            const uint4 v = *(const uint4*)(feats + row * D + c0);
            const float2 g = *(const float2*)(rowgrad + row * 2);
            const double gsh = (double)g.x, gsc = (double)g.y;
            const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double f0 = (double)__uint_as_float(wd[j] << 16), f1 = (double)__uint_as_float(wd[j] & 0xffff0000u);
                ash[2 * j] = ash[2 * j] + gsh * f0;
                ash[2 * j + 1] = ash[2 * j + 1] + gsh * f1;
                asc[2 * j] = asc[2 * j] + gsc * f0;
                asc[2 * j + 1] = asc[2 * j + 1] + gsc * f1;
            }
            bsh = bsh + gsh;
            bsc = bsc + gsc;
        }
    }
    double* out = part + (int64_t)(b * S + s) * (2 * D + 2);
    if (cl == 0) { s_b[rl][0] = bsh; s_b[rl][1] = bsc; }
#pragma unroll
    for (int which = 0; which < 2; which++) {           // (two rounds through an LDS tile of half the size: eight workgroups fit a CU, not four)
        if (which) __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; j++) s_acc[rl][cl][j] = which ? asc[j] : ash[j];
        __syncthreads();
        const int c = tid;                              // one of the block's 128 columns per thread
        if (c < 128 && cb * 128 + c < D) {
            double t = 0.0;
#pragma unroll
            for (int r = 0; r < 16; r++) t = t + s_acc[r][c >> 3][c & 7];
            out[(int64_t)which * D + cb * 128 + c] = t;
        }
    }
    if (cb == 0 && tid < 2) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 16; r++) t = t + s_b[r][tid];
        out[2 * D + tid] = t;
    }
}

// ---- the partials of an image added in chunk order, then the images' sums in image order, ONE rounding to f32 ---------------------------------------
// A workgroup owns 32 adjacent outputs (256 contiguous bytes of every partial); its 8 image lanes each add the S chunks of one image of a tile of
// eight, the eight sums go through LDS and image lane 0 adds them to the running total in ascending order.  (One thread per output over all B S
// partials is the same sum in a chain of B S dependent loads: 74 us at B S = 288, twice the partial-sum launch.)
__global__ __launch_bounds__(256) void ovb_head_finish_kernel(const double* __restrict__ part, float* dw_shift, float* dw_scale, float* db_shift,
                                                              float* db_scale, int D, int B, int S) {
    __shared__ double s_img[8][32];
    const int ol = threadIdx.x & 31, il = threadIdx.x >> 5;
    const int n = 2 * D + 2, o = blockIdx.x * 32 + ol;
    double tot = 0.0;
    for (int b0 = 0; b0 < B; b0 += 8) {                 // (block-uniform trip count: the barriers are reached by every thread)
        const int b = b0 + il;
        double t = 0.0;
        if (b < B && o < n) {
            const double* p = part + (int64_t)b * S * n + o;
#pragma unroll 4
            for (int s = 0; s < S; s++) t = t + p[(int64_t)s * n];
        }
        s_img[il][ol] = t;
        __syncthreads();
        if (il == 0) {
            const int nb = min(8, B - b0);
            for (int i = 0; i < nb; i++) tot = tot + s_img[i][ol];
        }
        __syncthreads();
    }
    if (il != 0 || o >= n) return;
    const float v = (float)tot;
    if (o < D) dw_shift[o] = v;
    else if (o < 2 * D) dw_scale[o - D] = v;
    else if (o == 2 * D) db_shift[0] = v;
    else db_scale[0] = v;
}

// rows of one dq^ partial slab: the image's rows in at most max(1, 64 / query blocks) chunks of a multiple of 32 rows -- a function of (P, Q) alone
static void ovb_split(int64_t P, int64_t Q, int* S, int* chunk) {
    const int nqb = (int)((Q + 31) / 32);
    const int s0 = nqb >= 64 ? 1 : 64 / nqb;
    const int64_t per = (P + s0 - 1) / s0;
    *chunk = (int)((per + 31) / 32 * 32);
    *S = (int)((P + *chunk - 1) / *chunk);
}

static int64_t ovb_align4(int64_t n) { return (n + 3) / 4 * 4; }

static int ovb_check_shape(const char* who, int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t Dt) {
    OWL_CHECK_ARG(B >= 1 && P >= 1 && P <= OVB_MAX_PATCHES && B * P < ((int64_t)1 << 31), "%s: B >= 1, 1 <= P <= %d and B P < 2^31 required (B=%lld P=%lld)", who,
                  OVB_MAX_PATCHES, (long long)B, (long long)P);
    OWL_CHECK_ARG(Q >= 1 && Q <= OVB_MAX_QUERIES, "%s: 1 <= Q <= %d required (Q=%lld)", who, OVB_MAX_QUERIES, (long long)Q);
    OWL_CHECK_ARG(Dt >= 64 && Dt % 64 == 0 && Dt <= 1024, "%s: Dt %% 64 == 0 and Dt <= 1024 required (Dt=%lld)", who, (long long)Dt);
    OWL_CHECK_ARG(nbanks == 1 || nbanks == B, "%s: queries is [nbanks, Q, Dt] with nbanks = B or 1 (got %lld for B=%lld)", who, (long long)nbanks, (long long)B);
    return 0;
}

// workspace (floats, every part a multiple of 4): q^ [nbanks Qp Dt], |q| and 1 / (|q| + eps) [nbanks Qp] each, rowfac [B P], and -- want_dq -- the slabs
OWL_API int owl_class_logits_bwd_workspace_bytes(int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t Dt, int want_dq, int64_t* bytes) {
    OWL_CHECK_ARG(bytes, "owl_class_logits_bwd_workspace_bytes: null pointer");
    if (ovb_check_shape("owl_class_logits_bwd_workspace_bytes", B, P, Q, nbanks, Dt)) return -1;
    const int64_t Qp = (Q + 31) / 32 * 32;
    int S, chunk;
    ovb_split(P, Q, &S, &chunk);
    int64_t n = nbanks * Qp * Dt + 2 * ovb_align4(nbanks * Qp) + ovb_align4(B * P);
    if (want_dq) n += B * S * Qp * Dt;
    *bytes = 4 * n;
    return 0;
}

// the launches of both entries; rowgrad (or null: owl_class_logits_bwd, whose launches and bits are what they were) receives (dshift, ds) per row
static int ovb_launch(const char* who, void* stream, const float* dlogits, const float* e, const float* queries, const float* w_shift, const float* w_scale,
                      const float* rowstats, const unsigned char* mask, void* workspace, void* de_bf16, float* dfeats, float* dqueries, float* rowgrad,
                      int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t nmasks, int64_t Dt, int64_t D) {
    OWL_CHECK_ARG(dlogits && e && queries && w_shift && w_scale && rowstats && workspace && de_bf16, "%s: null pointer", who);
    if (ovb_check_shape(who, B, P, Q, nbanks, Dt)) return -1;
    OWL_CHECK_ARG(D >= 8 && D % 8 == 0, "%s: D %% 8 == 0 required (D=%lld)", who, (long long)D);
    OWL_CHECK_ARG(!mask || nmasks == 1 || nmasks == B, "%s: mask is [nmasks, Q] with nmasks = B or 1 (got %lld for B=%lld)", who, (long long)nmasks,
                  (long long)B);
    OWL_CHECK_ARG((((uintptr_t)w_shift | (uintptr_t)w_scale | (uintptr_t)dfeats | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)rowstats & 7) == 0,
                  "%s: w_shift, w_scale, dfeats and workspace must be 16-byte aligned, rowstats 8-byte aligned", who);
    const int Qp = (int)((Q + 31) / 32 * 32), nqb = Qp / 32;
    int S, chunk;
    ovb_split(P, Q, &S, &chunk);
    OWL_CHECK_ARG(B * S * nqb < ((int64_t)1 << 31), "%s: B, P and Q together give too many workgroups for one launch", who);
    float* qhat = (float*)workspace;
    float* qnrm = qhat + nbanks * Qp * Dt;
    float* qinv = qnrm + ovb_align4(nbanks * Qp);
    float* rowfac = qinv + ovb_align4(nbanks * Qp);
    float* part = rowfac + ovb_align4(B * P);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ovb_qhat_kernel, dim3((unsigned)(nbanks * Qp)), dim3(64), 0, st, queries, qhat, qnrm, qinv, (int)Q, Qp, (int)Dt);
    OWL_LAUNCH_CHECK();
    const int tiles_img = (int)((P + 31) / 32);
    const dim3 grid((unsigned)(B * tiles_img));
    const int per_wave = (int)((Dt / 32 + 3) / 4);
#define OVB_ROWS(NT_)                                                                                                                              \
    hipLaunchKernelGGL(ovb_rows_kernel<NT_>, grid, dim3(256), 0, st, dlogits, e, qhat, rowstats, mask, w_shift, w_scale, (bf16_t*)de_bf16, dfeats, \
                       rowfac, rowgrad, (int)P, (int)Q, Qp, (int)Dt, (int)D, (int)nbanks, (int)nmasks, tiles_img)
#define OVB_DQ(NT_)                                                                                                                         \
    hipLaunchKernelGGL(ovb_dq_kernel<NT_>, dim3((unsigned)(B * S * nqb)), dim3(256), 0, st, dlogits, e, rowfac, mask, part, (int)P, (int)Q, Qp, \
                       (int)Dt, (int)nmasks, nqb, S, chunk)
    if (per_wave <= 1) OVB_ROWS(1);
    else if (per_wave <= 2) OVB_ROWS(2);
    else if (per_wave <= 4) OVB_ROWS(4);
    else if (per_wave <= 6) OVB_ROWS(6);
    else OVB_ROWS(8);
    OWL_LAUNCH_CHECK();
    if (!dqueries) return 0;
    if (per_wave <= 1) OVB_DQ(1);
    else if (per_wave <= 2) OVB_DQ(2);
    else if (per_wave <= 4) OVB_DQ(4);
    else if (per_wave <= 6) OVB_DQ(6);
    else OVB_DQ(8);
    OWL_LAUNCH_CHECK();
#undef OVB_ROWS
#undef OVB_DQ
    hipLaunchKernelGGL(ovb_dq_finish_kernel, dim3((unsigned)(nbanks * Q)), dim3(64), 0, st, part, queries, qhat, qnrm, qinv, dqueries, (int)Q, Qp, (int)Dt,
                       nbanks == 1 ? 0 : S, (int)(nbanks == 1 ? B * S : S));
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_class_logits_bwd(void* stream, const float* dlogits, const float* e, const float* queries, const float* w_shift, const float* w_scale,
                                 const float* rowstats, const unsigned char* mask, void* workspace, int64_t workspace_bytes, void* de_bf16, float* dfeats,
                                 float* dqueries, int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t nmasks, int64_t Dt, int64_t D) {
    OWL_CHECK_ARG(dlogits && e && queries && w_shift && w_scale && rowstats && workspace && de_bf16, "owl_class_logits_bwd: null pointer");
    if (ovb_check_shape("owl_class_logits_bwd", B, P, Q, nbanks, Dt)) return -1;
    OWL_CHECK_ARG(D >= 8 && D % 8 == 0, "owl_class_logits_bwd: D %% 8 == 0 required (D=%lld)", (long long)D);
    int64_t need = 0;
    if (owl_class_logits_bwd_workspace_bytes(B, P, Q, nbanks, Dt, dqueries != nullptr, &need)) return -1;
    OWL_CHECK_ARG(workspace_bytes >= need, "owl_class_logits_bwd: workspace of %lld bytes, %lld needed (owl_class_logits_bwd_workspace_bytes)",
                  (long long)workspace_bytes, (long long)need);
    return ovb_launch("owl_class_logits_bwd", stream, dlogits, e, queries, w_shift, w_scale, rowstats, mask, workspace, de_bf16, dfeats, dqueries, nullptr, B, P,
                      Q, nbanks, nmasks, Dt, D);
}

// workspace of owl_class_logits_bwd_head: owl_class_logits_bwd's, then the f64 partials [B S][2 D + 2] of the head gradients, S = ceil(P / OVB_HEAD_CHUNK)
OWL_API int owl_class_logits_bwd_head_workspace_bytes(int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t Dt, int64_t D, int want_dq, int64_t* bytes) {
    OWL_CHECK_ARG(bytes, "owl_class_logits_bwd_head_workspace_bytes: null pointer");
    if (ovb_check_shape("owl_class_logits_bwd_head_workspace_bytes", B, P, Q, nbanks, Dt)) return -1;
    OWL_CHECK_ARG(D >= 8 && D % 8 == 0 && D <= (1 << 20), "owl_class_logits_bwd_head_workspace_bytes: D %% 8 == 0 and D <= 2^20 required (D=%lld)", (long long)D);
    int64_t base = 0;
    if (owl_class_logits_bwd_workspace_bytes(B, P, Q, nbanks, Dt, want_dq, &base)) return -1;
    const int64_t S = (P + OVB_HEAD_CHUNK - 1) / OVB_HEAD_CHUNK;
    *bytes = base + 8 * B * S * (2 * D + 2);
    return 0;
}

OWL_API int owl_class_logits_bwd_head(void* stream, const float* dlogits, const float* e, const float* queries, const void* feats_bf16, const float* w_shift,
                                      const float* w_scale, const float* rowstats, const unsigned char* mask, void* workspace, int64_t workspace_bytes,
                                      float* rowgrad, void* de_bf16, float* dfeats, float* dqueries, float* dw_shift, float* dw_scale, float* db_shift,
                                      float* db_scale, int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t nmasks, int64_t Dt, int64_t D) {
    const char* who = "owl_class_logits_bwd_head";
    OWL_CHECK_ARG(dlogits && e && queries && feats_bf16 && w_shift && w_scale && rowstats && workspace && rowgrad && de_bf16 && dw_shift && dw_scale && db_shift &&
                      db_scale,
                  "%s: null pointer", who);
    int64_t need = 0, base = 0;
    if (owl_class_logits_bwd_head_workspace_bytes(B, P, Q, nbanks, Dt, D, dqueries != nullptr, &need)) return -1;
    if (owl_class_logits_bwd_workspace_bytes(B, P, Q, nbanks, Dt, dqueries != nullptr, &base)) return -1;
    OWL_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed (owl_class_logits_bwd_head_workspace_bytes)", who,
                  (long long)workspace_bytes, (long long)need);
    OWL_CHECK_ARG(((uintptr_t)feats_bf16 & 15) == 0 && ((uintptr_t)rowgrad & 7) == 0, "%s: feats must be 16-byte aligned, rowgrad 8-byte aligned", who);
    const int64_t S = (P + OVB_HEAD_CHUNK - 1) / OVB_HEAD_CHUNK, ncb = (D + 127) / 128;
    OWL_CHECK_ARG(B * S * ncb < ((int64_t)1 << 31) && B * S < ((int64_t)1 << 31), "%s: B, P and D together give too many workgroups for one launch", who);
    if (ovb_launch(who, stream, dlogits, e, queries, w_shift, w_scale, rowstats, mask, workspace, de_bf16, dfeats, dqueries, rowgrad, B, P, Q, nbanks, nmasks,
                   Dt, D))
        return -1;
    double* part = (double*)((char*)workspace + base);          // (base is a multiple of 16)
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ovb_head_part_kernel, dim3((unsigned)(B * S * ncb)), dim3(256), 0, st, (const bf16_t*)feats_bf16, rowgrad, part, (int)P, (int)D, (int)S,
                       (int)ncb);
    OWL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ovb_head_finish_kernel, dim3((unsigned)((2 * D + 2 + 31) / 32)), dim3(256), 0, st, part, dw_shift, dw_scale, db_shift, db_scale, (int)D,
                       (int)B, (int)S);
    OWL_LAUNCH_CHECK();
    return 0;
}
