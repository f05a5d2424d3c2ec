// Image-conditioned queries (OWL-ViT's `embed_image_query`, HF5 modeling_owlvit.py:1246-1288, extended to a query box inside the example image) and
// the query-bank fill that turns the selected class embeddings into `queries` rows.  Initialisation-time kernels: they run once, outside every step.
//
// owl_image_query_select, per exemplar n:
//   1. iou_p = HF box_iou(qbox, boxes_p) in f32, ONE rounding per written operation (this file is compiled with -ffp-contract=off, csrc/build.sh):
//      both areas, lt = max, rb = min, wh = clamp(rb - lt, 0), inter, union = (area_q + area_p) - inter, inter / union.
//   2. every iou_p == 0  ->  v_p = iou_p - (hull_p - union_p) / hull_p (HF generalized_box_iou); otherwise v_p = iou_p.
//   3. thr = fl32(max_p v_p * 0.8f), selected = {p : v_p >= thr}.  A negative maximum selects nothing (0.8 max > max): HF silently drops the image,
//      here the exemplar is reported EMPTY.  A NaN v_p (a box or hull of zero area) makes torch.max NaN and HF's selection empty: EMPTY here too.
//   4. mean_k = (sum over ALL p of e[p, k]) / P     5. sim_p = sum_k mean_k e[p, k], selected p     6. best = the selected p of smallest sim_p, the
//      LOWEST p on a tie (torch.argmin's first minimum).
// HF's quirks are kept, not fixed: the mean runs over all boxes while the argmin runs over the selected ones, the embeddings are NOT normalised, and
// after the fallback v_p <= 0 always, so a box is selected only when it touches the query box exactly (v_p == 0).
//
// Steps 4 to 6 accumulate in FLOAT64 (f32 inputs widened, f64 adds / FMAs, one fixed order), like owl_grad_sumsq and the mAP IoU: with f32 accumulation
// the worst-case error of a P-term column sum carried through a Dt-term dot is 1e-4 .. 5e-2 at P = 3600, Dt = 768 -- above the argmin margins random
// inputs show (2.5e-4 at the worst), so no derived bound could decide the argmin.  In f64 the bound is ~1e-13 and both kernels stay bandwidth-bound.
//
// Order of every sum (tests/image_query_reference.py counts exactly this):
//   column sum   image_query_colsum_kernel: workgroup (n, rb) adds rows 64 rb .. 64 rb + 63 of column k in ascending order (64 adds from 0) into
//                partial[n, rb, k]; the select kernel adds the partials in ascending rb (ceil(P / 64) adds from 0) and divides by P once.
//   dot          one wave per selected row: lane l runs acc = fma(mean_k, e_k, acc) over k = 256 j + 4 l + (0..3), j ascending, then the six
//                butterfly levels of common.h's wave_sum, in f64: 4 ceil(Dt / 256) + 6 links.
//   argmin       wave w takes the selected rows w, w + 4, ... in ascending p with a strict `<`; the four waves meet in order with (sim, p)
//                compared lexicographically: the lowest p among exact ties.
// No atomics, no host sync, nothing allocated; bitwise reproducible from run to run.
#include "common.h"

#define IQ_MAX_P 8192          // config.MAX_PATCHES: v_p and the selected list of one exemplar live in LDS
#define IQ_MAX_DT 1024         // mean (f64) and the bank row's accumulator live in LDS
#define IQ_ROWS 64             // rows per column-sum workgroup
#define IQ_THREADS 256
#define IQ_MAX_N (1 << 20)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// partial[n, rb, k] = sum of e[n, p, k] over p in [64 rb, min(64 rb + 64, P)), ascending, f64.  One thread per 4 columns (16 bytes per lane, a row
// contiguous across the lanes).
__global__ __launch_bounds__(IQ_THREADS) void image_query_colsum_kernel(const float* __restrict__ e, double* __restrict__ partial, int P, int Dt, int RB) {
    const int n = blockIdx.x / RB, rb = blockIdx.x % RB;
    const int p0 = rb * IQ_ROWS, p1 = min(p0 + IQ_ROWS, P);
    const float* src = e + (int64_t)n * P * Dt;
    double* dst = partial + ((int64_t)n * RB + rb) * Dt;
    for (int c = threadIdx.x * 4; c < Dt; c += IQ_THREADS * 4) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int p = p0; p < p1; p++) {
            const float4 v = *(const float4*)(src + (int64_t)p * Dt + c);
            a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
        }
        dst[c] = a0; dst[c + 1] = a1; dst[c + 2] = a2; dst[c + 3] = a3;
    }
}

struct IqBox { float x0, y0, x1, y1; };

// HF box_iou of one pair, f32, one rounding per written operation; `uni` returns the union
__device__ __forceinline__ float iq_iou(const IqBox& q, const float4& b, float& uni) {
#pragma clang fp contract(off)
    const float area_q = (q.x1 - q.x0) * (q.y1 - q.y0);
    const float area_p = (b.z - b.x) * (b.w - b.y);
    const float w = fmaxf(fminf(q.x1, b.z) - fmaxf(q.x0, b.x), 0.0f);
    const float h = fmaxf(fminf(q.y1, b.w) - fmaxf(q.y0, b.y), 0.0f);
    const float inter = w * h;
    uni = (area_q + area_p) - inter;
    return inter / uni;
}

__device__ __forceinline__ float iq_giou(const IqBox& q, const float4& b) {
#pragma clang fp contract(off)
    float uni;
    const float iou = iq_iou(q, b, uni);
    const float w = fmaxf(fmaxf(q.x1, b.z) - fminf(q.x0, b.x), 0.0f);
    const float h = fmaxf(fmaxf(q.y1, b.w) - fminf(q.y0, b.y), 0.0f);
    const float hull = w * h;
    return iou - (hull - uni) / hull;
}

// one workgroup (4 waves) per exemplar
__global__ __launch_bounds__(IQ_THREADS) void image_query_select_kernel(const float* __restrict__ e, const float* __restrict__ boxes,
                                                                         const float* __restrict__ qbox, const double* __restrict__ partial, int P, int Dt,
                                                                         int RB, int* __restrict__ best_out, float* __restrict__ query,
                                                                         int* __restrict__ info, float* __restrict__ v_out, double* __restrict__ mean_out,
                                                                         double* __restrict__ sim_out) {
    __shared__ float s_v[IQ_MAX_P];
    __shared__ unsigned short s_sel[IQ_MAX_P];
    __shared__ double s_mean[IQ_MAX_DT];
    __shared__ float s_wmax[4];
    __shared__ double s_wsim[4];
    __shared__ int s_widx[4];
    __shared__ int s_nsel, s_best;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* en = e + (int64_t)n * P * Dt;
    const float4* bn = (const float4*)(boxes + (int64_t)n * P * 4);
    IqBox q = {0.0f, 0.0f, 1.0f, 1.0f};
    if (qbox) {
        const float4 t = *(const float4*)(qbox + (int64_t)n * 4);
        q.x0 = t.x; q.y0 = t.y; q.x1 = t.z; q.y1 = t.w;
    }

    // 1. IoU; 2. the fallback when every IoU is exactly 0 (HF: torch.all(ious == 0.0); a NaN is not 0)
    int nonzero = 0;
    for (int p = tid; p < P; p += IQ_THREADS) {
        float uni;
        const float v = iq_iou(q, bn[p], uni);
        s_v[p] = v;
        nonzero |= !(v == 0.0f);
    }
    const int fallback = !__syncthreads_or(nonzero);
    if (fallback)
        for (int p = tid; p < P; p += IQ_THREADS) s_v[p] = iq_giou(q, bn[p]);          // (each thread rewrites the entries it wrote)

    // 3. the maximum (NaN -> empty), the threshold
    float m = -INFINITY;
    int nan = 0;
    for (int p = tid; p < P; p += IQ_THREADS) {
        const float v = s_v[p];
        nan |= (v != v);
        m = fmaxf(m, v);
        if (v_out) v_out[(int64_t)n * P + p] = v;
    }
    m = wave_max(m);
    if (lane == 0) s_wmax[wave] = m;
    const int any_nan = __syncthreads_or(nan);          // (also orders s_v and s_wmax)
    m = fmaxf(fmaxf(s_wmax[0], s_wmax[1]), fmaxf(s_wmax[2], s_wmax[3]));
    float thr;
    {
#pragma clang fp contract(off)
        thr = m * 0.8f;
    }

    // 4. mean_k: the partials in ascending row-block order, one division
    const double* pn = partial + (int64_t)n * RB * Dt;
    for (int k = tid; k < Dt; k += IQ_THREADS) {
        double s = 0.0;
        for (int rb = 0; rb < RB; rb++) s += pn[(int64_t)rb * Dt + k];
        s = s / (double)P;
        s_mean[k] = s;
        if (mean_out) mean_out[(int64_t)n * Dt + k] = s;
    }

    // the selected p, ascending, compacted by wave 0 (ballot + prefix count)
    if (wave == 0) {
        int cnt = 0;
        for (int base = 0; base < P; base += 64) {
            const int p = base + lane;
            const bool take = !any_nan && p < P && s_v[p] >= thr;
            const unsigned long long mask = __ballot(take);
            if (take) s_sel[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)p;
            cnt += __popcll(mask);
        }
        if (lane == 0) s_nsel = cnt;
    }
    if (sim_out)
        for (int p = tid; p < P; p += IQ_THREADS)
            if (any_nan || !(s_v[p] >= thr)) sim_out[(int64_t)n * P + p] = INFINITY;          // selected rows: written by the dot below
    __syncthreads();
    const int nsel = s_nsel;

    // 5. sim_p, one wave per selected row; 6. the running minimum (ascending p, strict <)
    double bsim = INFINITY;
    int bidx = -1;
    for (int j = wave; j < nsel; j += 4) {
        const int p = s_sel[j];
        const float* row = en + (int64_t)p * Dt;
        double acc = 0.0;
        for (int c = lane * 4; c < Dt; c += 256) {
            const float4 v = *(const float4*)(row + c);
            acc = fma(s_mean[c], (double)v.x, acc);
            acc = fma(s_mean[c + 1], (double)v.y, acc);
            acc = fma(s_mean[c + 2], (double)v.z, acc);
            acc = fma(s_mean[c + 3], (double)v.w, acc);
        }
        acc = wave_sum_f64(acc);
        if (sim_out && lane == 0) sim_out[(int64_t)n * P + p] = acc;
        if (bidx < 0 || acc < bsim) { bsim = acc; bidx = p; }
    }
    if (lane == 0) { s_wsim[wave] = bsim; s_widx[wave] = bidx; }
    __syncthreads();
    if (tid == 0) {
        double bs = 0.0;
        int bi = -1;
        for (int w = 0; w < 4; w++) {
            const int i = s_widx[w];
            if (i < 0) continue;
            const double s = s_wsim[w];
            if (bi < 0 || s < bs || (s == bs && i < bi)) { bs = s; bi = i; }
        }
        s_best = bi;
        best_out[n] = bi;
        info[2 * n] = (fallback ? 1 : 0) | (bi < 0 ? 2 : 0);
        info[2 * n + 1] = nsel;
    }
    __syncthreads();
    const int best = s_best;
    for (int c = tid * 4; c < Dt; c += IQ_THREADS * 4)
        *(float4*)(query + (int64_t)n * Dt + c) = best >= 0 ? *(const float4*)(en + (int64_t)best * Dt + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

static int64_t iq_row_blocks(int64_t P) { return (P + IQ_ROWS - 1) / IQ_ROWS; }

static int iq_check_shape(const char* who, int64_t N, int64_t P, int64_t Dt) {
    OWL_CHECK_ARG(N >= 1 && N <= IQ_MAX_N && P >= 1 && P <= IQ_MAX_P && Dt >= 4 && Dt % 4 == 0 && Dt <= IQ_MAX_DT,
                  "%s: N in 1 .. %d, P in 1 .. %d, Dt a positive multiple of 4 up to %d (got N = %lld, P = %lld, Dt = %lld)", who, IQ_MAX_N, IQ_MAX_P,
                  IQ_MAX_DT, (long long)N, (long long)P, (long long)Dt);
    return 0;
}

OWL_API int owl_image_query_workspace_bytes(int64_t N, int64_t P, int64_t Dt, int64_t* nbytes) {
    OWL_CHECK_ARG(nbytes, "owl_image_query_workspace_bytes: null pointer");
    if (iq_check_shape("owl_image_query_workspace_bytes", N, P, Dt)) return -1;
    *nbytes = N * iq_row_blocks(P) * Dt * (int64_t)sizeof(double);
    return 0;
}

OWL_API int owl_image_query_select(void* stream, const float* e, const float* boxes, const float* qbox, int64_t N, int64_t P, int64_t Dt, void* workspace,
                                   int64_t workspace_bytes, int* best, float* query, int* info, float* v_out, double* mean_out, double* sim_out) {
    OWL_CHECK_ARG(e && boxes && workspace && best && query && info, "owl_image_query_select: null pointer");
    if (iq_check_shape("owl_image_query_select", N, P, Dt)) return -1;
    const int64_t RB = iq_row_blocks(P);
    OWL_CHECK_ARG(workspace_bytes >= N * RB * Dt * (int64_t)sizeof(double),
                  "owl_image_query_select: workspace of %lld bytes, owl_image_query_workspace_bytes asks for %lld", (long long)workspace_bytes,
                  (long long)(N * RB * Dt * (int64_t)sizeof(double)));
    const int threads = (int)((Dt / 4 + 63) / 64 * 64) < IQ_THREADS ? (int)((Dt / 4 + 63) / 64 * 64) : IQ_THREADS;
    hipLaunchKernelGGL(image_query_colsum_kernel, dim3((unsigned)(N * RB)), dim3(threads), 0, (hipStream_t)stream, e, (double*)workspace, (int)P, (int)Dt,
                       (int)RB);
    OWL_LAUNCH_CHECK();
    hipLaunchKernelGGL(image_query_select_kernel, dim3((unsigned)N), dim3(IQ_THREADS), 0, (hipStream_t)stream, e, boxes, qbox, (const double*)workspace,
                       (int)P, (int)Dt, (int)RB, best, query, info, v_out, mean_out, sim_out);
    OWL_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// bank[r] = unit(sum over the members m of row r, ascending, of unit(query_m)), unit(x) = x / |x|: norms and sums in f64, ONE rounding to f32 at the
// store.  One workgroup per bank row; a row without members is not touched.  |x|^2: thread t runs ss = fma(x_k, x_k, ss) over k = 1024 j + 4 t + (0..3),
// the wave's butterfly, the four waves added in order.  A member index outside [0, N) is skipped (the host builds the table; nothing is read out of bounds).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_f64(double v, double* s_w) {
    v = wave_sum_f64(v);
    __syncthreads();          // (the previous use of s_w has been read)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(IQ_THREADS) void query_bank_fill_kernel(const float* __restrict__ query, const int* __restrict__ row_ptr,
                                                                      const int* __restrict__ members, float* __restrict__ bank, int N, int Dt) {
    __shared__ double s_acc[IQ_MAX_DT];
    __shared__ double s_w[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int m0 = row_ptr[r], m1 = row_ptr[r + 1];
    if (m1 <= m0) return;
    for (int k = tid; k < Dt; k += IQ_THREADS) s_acc[k] = 0.0;
    for (int i = m0; i < m1; i++) {
        const int m = members[i];
        if (m < 0 || m >= N) continue;          // (uniform over the workgroup)
        const float* x = query + (int64_t)m * Dt;
        double ss = 0.0;
        for (int c = tid * 4; c < Dt; c += IQ_THREADS * 4) {
            const float4 v = *(const float4*)(x + c);
            ss = fma((double)v.x, (double)v.x, ss); ss = fma((double)v.y, (double)v.y, ss);
            ss = fma((double)v.z, (double)v.z, ss); ss = fma((double)v.w, (double)v.w, ss);
        }
        const double nrm = sqrt(block_sum_f64(ss, s_w));
        for (int c = tid * 4; c < Dt; c += IQ_THREADS * 4) {          // (a thread owns the same columns in every loop: no barrier between them)
            const float4 v = *(const float4*)(x + c);
            s_acc[c] += (double)v.x / nrm; s_acc[c + 1] += (double)v.y / nrm; s_acc[c + 2] += (double)v.z / nrm; s_acc[c + 3] += (double)v.w / nrm;
        }
    }
    double ss = 0.0;
    for (int c = tid * 4; c < Dt; c += IQ_THREADS * 4)
        for (int i = 0; i < 4; i++) ss = fma(s_acc[c + i], s_acc[c + i], ss);
    const double nrm = sqrt(block_sum_f64(ss, s_w));
    for (int c = tid * 4; c < Dt; c += IQ_THREADS * 4)
        *(float4*)(bank + (int64_t)r * Dt + c) = make_float4((float)(s_acc[c] / nrm), (float)(s_acc[c + 1] / nrm), (float)(s_acc[c + 2] / nrm), (float)(s_acc[c + 3] / nrm));
}

OWL_API int owl_query_bank_fill(void* stream, const float* query, const int* row_ptr, const int* members, float* bank, int64_t N, int64_t nq, int64_t Dt) {
    OWL_CHECK_ARG(query && row_ptr && members && bank, "owl_query_bank_fill: null pointer");
    OWL_CHECK_ARG(N >= 1 && N <= IQ_MAX_N && nq >= 1 && nq <= 3 * OWL_WIDE_MAX_CLASSES && Dt >= 4 && Dt % 4 == 0 && Dt <= IQ_MAX_DT,
                  "owl_query_bank_fill: N in 1 .. %d, nq in 1 .. %d, Dt a positive multiple of 4 up to %d (got N = %lld, nq = %lld, Dt = %lld)", IQ_MAX_N,
                  3 * OWL_WIDE_MAX_CLASSES, IQ_MAX_DT, (long long)N, (long long)nq, (long long)Dt);
    hipLaunchKernelGGL(query_bank_fill_kernel, dim3((unsigned)nq), dim3(IQ_THREADS), 0, (hipStream_t)stream, query, row_ptr, members, bank, (int)N, (int)Dt);
    OWL_LAUNCH_CHECK();
    return 0;
}
