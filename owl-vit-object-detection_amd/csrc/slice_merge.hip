// Sliced inference, the merge (postprocess.SlicedPostProcess): the candidates owl_postprocess left on T slices -- (box, score, class) records with
// per-slice counts -- become one detection list per SOURCE image.  Compiled with -ffp-contract=off: the slice -> image map is one f32 multiply and
// one f32 add per coordinate, and the overlap compare sees the IEEE f32 results tests/slice_merge_reference.py bounds.
//
//   per source image g (slices slice_offsets[g] .. slice_offsets[g + 1], a CSR: the groups are ragged):
//               candidate c = local_slice * K + rank, live iff rank < counts[slice] and its score is not NaN
//               box mapped into the full image:  x = ox + bx * sx,  y = oy + by * sy  (xform row (sx, ox, sy, oy) of its slice), never clipped
//               order: score descending, then c ascending; -0.0 == +0.0; the emitted score keeps the input's bits
//               greedy suppression, same class (or any class: class_aware == 0), ovr > thr, with
//                  metric 0  ovr = inter / (ai + aj - inter)      -- pp_mask_kernel's per-class route, operation for operation
//                  metric 1  ovr = inter / fminf(ai, aj)          -- intersection over the smaller: a box cut by a slice border against the whole box
//                  0 / 0 is NaN and suppresses nothing
//               optional prefix of max_out
//
// Three launches, no host sync, no global atomics, nothing allocated -- the structure of postprocess.hip:
//   sm_sort_kernel   one 1024-thread workgroup per source image: 64-bit keys (score desc | c asc) bitonic-sorted in LDS, then the sorted candidates'
//                    mapped boxes, scores, classes and c written out
//   sm_mask_kernel   one wave per 64x64 block of the sorted pair matrix: bit t of word [i][cb] = "candidate i suppresses candidate cb*64+t"
//   sm_scan_kernel   one wave per source image walks the sorted list with a 128-word "removed" set (two u64 per lane), mask rows fetched 8 ahead
#include "common.h"

typedef unsigned long long u64;

__device__ __forceinline__ unsigned sm_orderable(float f) {   // monotone map f32 -> u32
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// slices of group g, clamped to the arrays' extents: a malformed CSR reads and writes nothing out of bounds
__device__ __forceinline__ void sm_group(const int* __restrict__ slice_offsets, int g, int T, int K, int N, int& s0, int& n_cand) {
    s0 = min(max(slice_offsets[g], 0), T);
    const int s1 = min(max(slice_offsets[g + 1], s0), T);
    n_cand = (int)min((int64_t)(s1 - s0) * K, (int64_t)N);
}

template <int NP>
__global__ __launch_bounds__(1024) void sm_sort_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                       const int64_t* __restrict__ classes, const int* __restrict__ counts,
                                                       const float* __restrict__ xform, const int* __restrict__ slice_offsets,
                                                       float* __restrict__ s_box, float* __restrict__ s_score, int64_t* __restrict__ s_cls,
                                                       int* __restrict__ s_idx, int* __restrict__ n_valid, int T, int K, int N) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* keys = (u64*)smem;
    const int g = blockIdx.x, tid = threadIdx.x;
    int s0, n_cand;
    sm_group(slice_offsets, g, T, K, N, s0, n_cand);
    for (int p = tid; p < NP; p += 1024) {
        u64 key = ~0ull;
        if (p < n_cand) {
            const int sl = s0 + p / K, rank = p % K;
            if (rank < counts[sl]) {
                const float v = scores[(int64_t)sl * K + rank];
                // -0.0 == +0.0 in the order (c breaks the tie): both zeros take +0.0's key
                if (v == v) key = ((u64)(~sm_orderable(v == 0.f ? 0.f : v)) << 32) | (u64)(unsigned)p;
            }
        }
        keys[p] = key;
    }
    __syncthreads();
    for (int k = 2; k <= NP; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < NP / 2; t += 1024) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const u64 a = keys[i], c = keys[l];
                const bool up = (i & k) == 0;
                if ((a > c) == up) { keys[i] = c; keys[l] = a; }
            }
            __syncthreads();
        }
    }
    if (tid == 0 && keys[0] == ~0ull) n_valid[g] = 0;
    for (int p = tid; p < n_cand; p += 1024) {
        const u64 key = keys[p];
        if (key == ~0ull) continue;
        const int c = (int)(unsigned)(key & 0xFFFFFFFFull);
        const int sl = s0 + c / K;
        const int64_t in = (int64_t)sl * K + c % K;
        const int64_t o = (int64_t)g * N + p;
        const float4 bx = ((const float4*)boxes)[in];
        const float4 xf = ((const float4*)xform)[sl];           // (sx, ox, sy, oy)
        float4 m;                                               // a multiply, then an add (-ffp-contract=off), as the reference maps them
        m.x = xf.y + bx.x * xf.x;
        m.y = xf.w + bx.y * xf.z;
        m.z = xf.y + bx.z * xf.x;
        m.w = xf.w + bx.w * xf.z;
        ((float4*)s_box)[o] = m;
        s_score[o] = scores[in];                                // the input's own bits (the key holds one zero for both)
        s_cls[o] = classes[in];
        s_idx[o] = c;
        if (p + 1 == n_cand || keys[p + 1] == ~0ull) n_valid[g] = p + 1;
    }
}

__global__ __launch_bounds__(64) void sm_mask_kernel(const float* __restrict__ s_box, const int64_t* __restrict__ s_cls,
                                                     const int* __restrict__ n_valid, u64* __restrict__ mask, int N, int W, float thr,
                                                     int metric, int class_aware) {
    const int cb = blockIdx.x, rb = blockIdx.y, g = blockIdx.z, lane = threadIdx.x;
    const int n = n_valid[g];
    const int i = rb * 64 + lane;
    if (rb * 64 >= n) return;                       // rows >= n_valid are never read by the scan
    u64 bits = 0;
    if (cb >= rb && cb * 64 < n) {
        const int64_t base = (int64_t)g * N;
        const int ii = min(i, N - 1), jj = min(cb * 64 + lane, N - 1);
        const float4 bi = ((const float4*)s_box)[base + ii];
        const float4 bj = ((const float4*)s_box)[base + jj];
        const int64_t ci = class_aware ? s_cls[base + ii] : 0;
        const int64_t cj = class_aware ? s_cls[base + jj] : 0;
        const int cjl = (int)(unsigned)(u64)cj, cjh = (int)(unsigned)((u64)cj >> 32);
        const float ai = (bi.z - bi.x) * (bi.w - bi.y);
        const float aj = (bj.z - bj.x) * (bj.w - bj.y);
#pragma unroll
        for (int t = 0; t < 64; t++) {
            const float x1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bj.x), t));
            const float y1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bj.y), t));
            const float x2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bj.z), t));
            const float y2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, bj.w), t));
            const float at = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, aj), t));
            const unsigned ctl = (unsigned)__builtin_amdgcn_readlane(cjl, t), cth = (unsigned)__builtin_amdgcn_readlane(cjh, t);
            const int64_t ct = (int64_t)(((u64)cth << 32) | ctl);
            const int j = cb * 64 + t;
            const float w = fmaxf(0.f, fminf(bi.z, x2) - fmaxf(bi.x, x1));
            const float h = fmaxf(0.f, fminf(bi.w, y2) - fmaxf(bi.y, y1));
            const float inter = w * h;
            const float ovr = metric ? inter / fminf(ai, at) : inter / (ai + at - inter);
            if (j > i && j < n && ct == ci && ovr > thr) bits |= 1ull << t;
        }
    }
    if (i < n) mask[((int64_t)g * N + i) * W + cb] = bits;
}

__global__ __launch_bounds__(64) void sm_scan_kernel(const u64* __restrict__ mask, const float* __restrict__ s_box,
                                                     const float* __restrict__ s_score, const int64_t* __restrict__ s_cls,
                                                     const int* __restrict__ s_idx, const int* __restrict__ n_valid,
                                                     float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                     int64_t* __restrict__ out_classes, int64_t* __restrict__ out_src,
                                                     int* __restrict__ out_count, int N, int W, int max_out) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int n = n_valid[g];
    const u64* m = mask + (int64_t)g * N * W;
    const int64_t base = (int64_t)g * N;
    u64 remv0 = 0, remv1 = 0;
    int kept = 0;
    for (int i0 = 0; i0 < n && kept < max_out; i0 += 8) {
        u64 r0[8], r1[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int row = min(i0 + u, n - 1);
            r0[u] = lane < W ? m[(int64_t)row * W + lane] : 0ull;
            r1[u] = lane + 64 < W ? m[(int64_t)row * W + lane + 64] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int i = i0 + u;
            if (i < n && kept < max_out) {
                const int w = i >> 6;
                const u64 src = w < 64 ? remv0 : remv1;
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)src, w & 63);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(src >> 32), w & 63);
                const u64 word = ((u64)hi << 32) | lo;
                if (!((word >> (i & 63)) & 1ull)) {
                    if (lane == 0) {
                        const int64_t o = (int64_t)g * max_out + kept;
                        ((float4*)out_boxes)[o] = ((const float4*)s_box)[base + i];
                        out_scores[o] = s_score[base + i];
                        out_classes[o] = s_cls[base + i];
                        out_src[o] = s_idx[base + i];
                    }
                    kept++;
                    remv0 |= r0[u];
                    remv1 |= r1[u];
                }
            }
        }
    }
    if (lane == 0) out_count[g] = kept;
}

// s_box [G,N,4] f32 | s_cls [G,N] i64 | s_score [G,N] f32 | s_idx [G,N] i32 | (256-byte boundary) mask [G,N,W] u64 | n_valid [G] i32
static int64_t sm_ws_bytes(int64_t G, int64_t N) {
    const int64_t W = (N + 63) / 64;
    return G * N * (16 + 8 + 4 + 4) + 256 + G * N * W * 8 + G * 4 + 256;
}

OWL_API int owl_slice_merge_workspace(int64_t G, int64_t Nmax, int64_t* bytes) {
    OWL_CHECK_ARG(G > 0 && G <= 65535 && Nmax > 0 && Nmax <= 8192 && bytes, "owl_slice_merge_workspace: need 0 < G <= 65535, 0 < Nmax <= 8192 (G=%lld Nmax=%lld)", (long long)G, (long long)Nmax);
    *bytes = sm_ws_bytes(G, Nmax);
    return 0;
}

OWL_API int owl_slice_merge(void* stream, const float* boxes, const float* scores, const int64_t* classes, const int* counts,
                            const float* xform, const int* slice_offsets, void* workspace, int64_t ws_bytes,
                            float* out_boxes, float* out_scores, int64_t* out_classes, int64_t* out_src, int* out_count,
                            int64_t T, int64_t K, int64_t G, int64_t Nmax, int64_t max_out, float thr, int metric, int class_aware) {
    OWL_CHECK_ARG(boxes && scores && classes && counts && xform && slice_offsets && workspace && out_boxes && out_scores && out_classes && out_src && out_count,
                  "owl_slice_merge: null pointer");
    OWL_CHECK_ARG(T > 0 && K > 0 && G > 0 && G <= 65535 && T * K < (1ll << 31) && max_out > 0 && max_out < (1ll << 31),
                  "owl_slice_merge: need T > 0, K > 0, 0 < G <= 65535, max_out > 0 (T=%lld K=%lld G=%lld max_out=%lld)", (long long)T, (long long)K, (long long)G, (long long)max_out);
    OWL_CHECK_ARG(Nmax >= K && Nmax <= 8192, "owl_slice_merge: need K <= Nmax <= 8192 candidates per source image, the ceiling of the LDS sort and of the scan's 128 mask words (K=%lld Nmax=%lld)", (long long)K, (long long)Nmax);
    OWL_CHECK_ARG(metric == 0 || metric == 1, "owl_slice_merge: metric must be 0 (intersection over union) or 1 (intersection over the smaller area)");
    OWL_CHECK_ARG(class_aware == 0 || class_aware == 1, "owl_slice_merge: class_aware must be 0 or 1");
    OWL_CHECK_ARG(ws_bytes >= sm_ws_bytes(G, Nmax), "owl_slice_merge: workspace %lld < required %lld bytes", (long long)ws_bytes, (long long)sm_ws_bytes(G, Nmax));
    OWL_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)boxes & 15) == 0 && ((uintptr_t)xform & 15) == 0 && ((uintptr_t)out_boxes & 15) == 0,
                  "owl_slice_merge: boxes / xform / out_boxes / workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int N = (int)Nmax, W = (N + 63) / 64;
    unsigned char* ws = (unsigned char*)workspace;
    float* s_box = (float*)ws;                 ws += G * N * 16;
    int64_t* s_cls = (int64_t*)ws;             ws += G * N * 8;
    float* s_score = (float*)ws;               ws += G * N * 4;
    int* s_idx = (int*)ws;                     ws += G * N * 4;
    ws = (unsigned char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    u64* mask = (u64*)ws;                      ws += G * N * (int64_t)W * 8;
    int* n_valid = (int*)ws;
    if (N <= 1024) hipLaunchKernelGGL((sm_sort_kernel<1024>), dim3((unsigned)G), dim3(1024), 1024 * 8, s, boxes, scores, classes, counts, xform, slice_offsets, s_box, s_score, s_cls, s_idx, n_valid, (int)T, (int)K, N);
    else if (N <= 4096) hipLaunchKernelGGL((sm_sort_kernel<4096>), dim3((unsigned)G), dim3(1024), 4096 * 8, s, boxes, scores, classes, counts, xform, slice_offsets, s_box, s_score, s_cls, s_idx, n_valid, (int)T, (int)K, N);
    else hipLaunchKernelGGL((sm_sort_kernel<8192>), dim3((unsigned)G), dim3(1024), 8192 * 8, s, boxes, scores, classes, counts, xform, slice_offsets, s_box, s_score, s_cls, s_idx, n_valid, (int)T, (int)K, N);
    OWL_LAUNCH_CHECK();
    hipLaunchKernelGGL(sm_mask_kernel, dim3(W, W, (unsigned)G), dim3(64), 0, s, s_box, s_cls, n_valid, mask, N, W, thr, metric, class_aware);
    OWL_LAUNCH_CHECK();
    hipLaunchKernelGGL(sm_scan_kernel, dim3((unsigned)G), dim3(64), 0, s, mask, s_box, s_score, s_cls, s_idx, n_valid, out_boxes, out_scores, out_classes, out_src, out_count, N, W, (int)max_out);
    OWL_LAUNCH_CHECK();
    return 0;
}
