// COCO bbox mAP on device: the metric of the reference's eval loop (ref main.py:31,120-128,144; src/train_util.py:37-64 ->
// torchmetrics MeanAveragePrecision(iou_type="bbox") -> pycocotools COCOeval evaluateImg / accumulate).  Compiled with -ffp-contract=off:
// the f32 box scaling and the f64 IoU / precision arithmetic are IEEE operation by operation, so every comparison against a threshold sees the
// value the host protocol sees.  The protocol's constants (IoU / recall thresholds, area ranges, maxDets, eps) arrive as arrays from the
// caller and are never re-derived here.
//
//   map_match_kernel       one launch per metric update, one wave per (image, class) + one wave per image for the slots that are no records.
//                          The class's detections are compacted into LDS in slot order, ranked by (score descending, slot ascending) and cut to
//                          100; its ground truths are ordered non-ignored first per area range.  Lane a * 10 + t then runs the greedy matching
//                          chain of area range a and IoU threshold t over the detections in rank order (the 40 chains are independent; each is
//                          sequential): boxes in LDS, f64 IoU recomputed per pair, one "taken" byte per (ground-truth position, lane) in LDS.
//                          A ballot per detection packs the 40 matched / ignored bits into four 20-bit words.
//   map_accumulate_kernel  one launch per compute(), one wave per (class, area range, maxDet, IoU threshold) over the class's records (sorted by
//                          descending score by the caller): pass 1 counts tp / fp, pass 2 walks the records backwards in chunks of 64 --
//                          ballot prefix counts give the integer cumulative sums, f64 divisions the precision / recall, a shuffle scan the
//                          running maximum from the right; the entry at which recall first reaches a threshold writes that threshold's
//                          precision (= searchsorted(rc, thr, 'left') without storing rc).  No atomics, no scratch.
#include "common.h"

typedef unsigned long long u64;

#define MAP_T 10            // IoU thresholds (bits per mask word)
#define MAP_A 4             // area ranges
#define MAP_M 3             // maxDets
#define MAP_R 101           // recall thresholds
#define MAP_MAXDET 100      // detections kept per (image, class) = the largest maxDet
#define MAP_KMAX 1024       // detection slots per image
#define MAP_GMAX 256        // ground-truth slots per image

__device__ __forceinline__ u64 lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

__global__ __launch_bounds__(64) void map_match_kernel(const float* __restrict__ det_boxes, const float* __restrict__ det_scores,
                                                       const int64_t* __restrict__ det_labels, const int* __restrict__ det_counts,
                                                       const float* __restrict__ gt_boxes, const int64_t* __restrict__ gt_labels,
                                                       const int* __restrict__ gt_counts, const float* __restrict__ scale,
                                                       const double* __restrict__ iou_thr, const double* __restrict__ area_rng,
                                                       float* __restrict__ rec_score, int64_t* __restrict__ rec_label, int* __restrict__ rec_rank,
                                                       int* __restrict__ rec_mask, int* __restrict__ npig, int K, int G, int C) {
    __shared__ float c_score[MAP_KMAX];                 // the class's detections, slot order
    __shared__ unsigned short c_slot[MAP_KMAX];
    __shared__ unsigned short d_ord[MAP_MAXDET];        // rank -> candidate
    __shared__ float4 d_box[MAP_MAXDET];                // xywh, f32
    __shared__ float4 g_box[MAP_GMAX];                  // the class's ground truths, arrival order
    __shared__ unsigned char g_ord[MAP_A][MAP_GMAX];    // per area range: position -> ground truth, non-ignored first
    __shared__ unsigned char g_taken[MAP_GMAX * 64];    // [position][lane]
    const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int64_t dbase = (int64_t)b * K;
    const int nslots = min(max(det_counts[b], 0), K);

    if (c == C) {       // every slot that holds no detection of a class in [0, C): padding or a label out of range
        for (int i = lane; i < K; i += 64) {
            const int64_t lab = i < nslots ? det_labels[dbase + i] : -1;
            if (lab < 0 || lab >= C) {
                rec_score[dbase + i] = 0.f; rec_label[dbase + i] = -1; rec_rank[dbase + i] = 0;
                for (int a = 0; a < MAP_A; a++) rec_mask[(dbase + i) * MAP_A + a] = 0;
            }
        }
        return;
    }

    // ---- detections of class c, in slot order
    int n = 0;
    for (int i0 = 0; i0 < nslots; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < nslots && det_labels[dbase + i] == (int64_t)c;
        const u64 bal = __ballot(mine);
        if (mine) {
            const int pos = n + __popcll(bal & lanes_below(lane));
            c_slot[pos] = (unsigned short)i;
            c_score[pos] = det_scores[dbase + i];
        }
        n += __popcll(bal);
    }
    __syncthreads();
    // ---- rank = position under the stable sort by descending score; the first 100 are the records
    for (int p = lane; p < n; p += 64) {
        const float s = c_score[p];
        int r = 0;
        for (int q = 0; q < n; q++) {
            const float sq = c_score[q];
            r += (sq > s || (sq == s && q < p)) ? 1 : 0;
        }
        const int64_t o = dbase + c_slot[p];
        if (r < MAP_MAXDET) {
            d_ord[r] = (unsigned short)p;
            rec_score[o] = s; rec_label[o] = c; rec_rank[o] = r;
        } else {
            rec_score[o] = 0.f; rec_label[o] = -1; rec_rank[o] = 0;
            for (int a = 0; a < MAP_A; a++) rec_mask[o * MAP_A + a] = 0;
        }
    }
    const int nd = min(n, MAP_MAXDET);
    const float sx = scale[2 * b], sy = scale[2 * b + 1];
    __syncthreads();
    for (int r = lane; r < nd; r += 64) {
        const float* bx = det_boxes + (dbase + c_slot[d_ord[r]]) * 4;
        const float x0 = bx[0] * sx, y0 = bx[1] * sy, x1 = bx[2] * sx, y1 = bx[3] * sy;
        d_box[r] = make_float4(x0, y0, x1 - x0, y1 - y0);
    }
    // ---- ground truths of class c, arrival order
    const int64_t gbase = (int64_t)b * G;
    const int ngslots = min(max(gt_counts[b], 0), G);
    int ng = 0;
    for (int j0 = 0; j0 < ngslots; j0 += 64) {
        const int j = j0 + lane;
        const bool mine = j < ngslots && gt_labels[gbase + j] == (int64_t)c;
        const u64 bal = __ballot(mine);
        if (mine) {
            const float* bx = gt_boxes + (gbase + j) * 4;
            const float x0 = bx[0] * sx, y0 = bx[1] * sy, x1 = bx[2] * sx, y1 = bx[3] * sy;
            g_box[ng + __popcll(bal & lanes_below(lane))] = make_float4(x0, y0, x1 - x0, y1 - y0);
        }
        ng += __popcll(bal);
    }
    __syncthreads();
    // ---- per area range: non-ignored ground truths first, each group in arrival order
    int nv[MAP_A];
#pragma unroll
    for (int a = 0; a < MAP_A; a++) {
        const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
        int cnt = 0;
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            for (int j0 = 0; j0 < ng; j0 += 64) {
                const int j = j0 + lane;
                bool f = false;
                if (j < ng) {
                    const float4 g = g_box[j];
                    const double area = (double)g.z * (double)g.w;
                    f = (area < lo || area > hi) == (pass == 1);
                }
                const u64 bal = __ballot(f);
                if (f) g_ord[a][cnt + __popcll(bal & lanes_below(lane))] = (unsigned char)j;
                cnt += __popcll(bal);
            }
            if (pass == 0) nv[a] = cnt;
        }
    }
    if (lane < MAP_A) {
        int v = nv[0];
#pragma unroll
        for (int a = 1; a < MAP_A; a++) v = lane == a ? nv[a] : v;
        npig[((int64_t)b * C + c) * MAP_A + lane] = v;
    }
    for (int p = 0; p < ng; p++) g_taken[p * 64 + lane] = 0;
    __syncthreads();
    // ---- the 40 matching chains
    const bool chain = lane < MAP_A * MAP_T;
    const int a = chain ? lane / MAP_T : 0, t = chain ? lane % MAP_T : 0;
    const double thr = fmin(iou_thr[t], 1.0 - 1e-10);
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    int nva = nv[0];
#pragma unroll
    for (int k = 1; k < MAP_A; k++) nva = a == k ? nv[k] : nva;
    for (int r = 0; r < nd; r++) {
        const float4 df = d_box[r];
        const double dx = df.x, dy = df.y, dw = df.z, dh = df.w;
        const double da = dw * dh;
        double best = thr;
        int m = -1;
        bool stop = !chain;
        for (int p = 0; p < ng; p++) {
            if (!__any(!stop)) break;
            bool open = !stop && !g_taken[p * 64 + lane];
            if (open && m >= 0 && m < nva && p >= nva) { stop = true; open = false; }   // a non-ignored match is never traded for an ignored ground truth
            if (open) {
                const float4 gf = g_box[g_ord[a][p]];
                const double gx = gf.x, gy = gf.y, gw = gf.z, gh = gf.w;
                const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
                const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
                double iou = 0.0;
                if (iw > 0 && ih > 0) {
                    const double inter = iw * ih;
                    iou = inter / (da + gw * gh - inter);
                }
                if (!(iou < best)) { best = iou; m = p; }                      // equal IoU moves the match to the later ground truth
            }
        }
        const bool matched = chain && m >= 0;
        if (matched) g_taken[m * 64 + lane] = 1;
        const bool ign = chain && (matched ? m >= nva : (da < lo || da > hi));
        const u64 bm = __ballot(matched), bi = __ballot(ign);
        if (lane < MAP_A) {
            const unsigned w = (unsigned)((bm >> (lane * MAP_T)) & 0x3ffu) | ((unsigned)((bi >> (lane * MAP_T)) & 0x3ffu) << MAP_T);
            rec_mask[(dbase + c_slot[d_ord[r]]) * MAP_A + lane] = (int)w;
        }
    }
}

// #{r : rec_thr[r] <= x}, rec_thr ascending
__device__ __forceinline__ int thr_reached(const double* thr, double x) {
    int lo = 0, hi = MAP_R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void map_accumulate_kernel(const int* __restrict__ rec_rank, const int* __restrict__ rec_mask,
                                                            const int64_t* __restrict__ seg, const int* __restrict__ npig,
                                                            const double* __restrict__ rec_thr, const int* __restrict__ max_dets, double eps,
                                                            double* __restrict__ precision, double* __restrict__ recall, int C) {
    __shared__ double thr[MAP_R];
    const int lane = threadIdx.x, k = blockIdx.y;
    const int t = blockIdx.x % MAP_T, am = blockIdx.x / MAP_T, a = am / MAP_M, mi = am % MAP_M;
    const int64_t pstride = (int64_t)C * MAP_A * MAP_M;                         // precision[t][r][k][a][m]
    double* prec = precision + (int64_t)t * MAP_R * pstride + ((int64_t)k * MAP_A + a) * MAP_M + mi;
    double* rec = recall + (((int64_t)t * C + k) * MAP_A + a) * MAP_M + mi;
    const int np = npig[k * MAP_A + a];
    if (np <= 0) {
        for (int r = lane; r < MAP_R; r += 64) prec[r * pstride] = -1.0;
        if (lane == 0) *rec = -1.0;
        return;
    }
    for (int r = lane; r < MAP_R; r += 64) thr[r] = rec_thr[r];
    __syncthreads();
    const int64_t s0 = seg[k], s1 = seg[k + 1];
    const int64_t n = s1 > s0 ? s1 - s0 : 0;
    const int maxdet = max_dets[mi];
    const int nchunks = (int)((n + 63) / 64);
    int tot_tp = 0, tot_fp = 0;
    for (int ch = 0; ch < nchunks; ch++) {
        const int64_t i = s0 + (int64_t)ch * 64 + lane;
        bool tp = false, fp = false;
        if (i < s1 && rec_rank[i] < maxdet) {
            const unsigned w = (unsigned)rec_mask[i * MAP_A + a];
            const bool mt = (w >> t) & 1u, ig = (w >> (MAP_T + t)) & 1u;
            tp = mt && !ig; fp = !mt && !ig;
        }
        tot_tp += __popcll(__ballot(tp));
        tot_fp += __popcll(__ballot(fp));
    }
    const double npd = (double)np;
    if (lane == 0) *rec = n > 0 ? (double)tot_tp / npd : 0.0;
    // recall thresholds the curve never reaches
    for (int r = (n > 0 ? thr_reached(thr, (double)tot_tp / npd) : 0) + lane; r < MAP_R; r += 64) prec[r * pstride] = 0.0;
    int suf_tp = 0, suf_fp = 0;
    double carry = 0.0;                                                         // running maximum from the right (precisions are >= 0)
    for (int ch = nchunks - 1; ch >= 0; ch--) {
        const int64_t i = s0 + (int64_t)ch * 64 + lane;
        const bool valid = i < s1;
        bool tp = false, fp = false;
        if (valid && rec_rank[i] < maxdet) {
            const unsigned w = (unsigned)rec_mask[i * MAP_A + a];
            const bool mt = (w >> t) & 1u, ig = (w >> (MAP_T + t)) & 1u;
            tp = mt && !ig; fp = !mt && !ig;
        }
        const u64 btp = __ballot(tp), bfp = __ballot(fp);
        const int ctp = __popcll(btp), cfp = __popcll(bfp);
        const u64 upto = lanes_below(lane) | (1ull << lane);
        const int tpi = tot_tp - suf_tp - ctp + __popcll(btp & upto);          // inclusive cumulative sums at this record
        const int fpi = tot_fp - suf_fp - cfp + __popcll(bfp & upto);
        double v = valid ? (double)tpi / ((double)(fpi + tpi) + eps) : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_down(v, o, 64);
            if (lane + o < 64) v = fmax(v, u);
        }
        v = fmax(v, carry);
        carry = __shfl(v, 0, 64);
        if (valid && (tp || i == s0)) {       // recall changes here: this record is searchsorted(rc, thr, 'left') for the thresholds in (rc before, rc here]
            const int r0 = i == s0 ? 0 : thr_reached(thr, (double)(tpi - 1) / npd);
            const int r1 = thr_reached(thr, (double)tpi / npd);
            for (int r = r0; r < r1; r++) prec[r * pstride] = v;
        }
        suf_tp += ctp; suf_fp += cfp;
    }
}

OWL_API int owl_map_match(void* stream, const float* det_boxes, const float* det_scores, const int64_t* det_labels, const int* det_counts,
                          const float* gt_boxes, const int64_t* gt_labels, const int* gt_counts, const float* scale, const double* iou_thr,
                          const double* area_rng, float* rec_score, int64_t* rec_label, int* rec_rank, int* rec_mask, int* npig,
                          int64_t B, int64_t K, int64_t G, int64_t C) {
    OWL_CHECK_ARG(K > 0 && K <= MAP_KMAX && G > 0 && G <= MAP_GMAX, "owl_map_match: need 0 < K <= %d detection slots and 0 < G <= %d ground-truth slots per image (K=%lld G=%lld)", MAP_KMAX, MAP_GMAX, (long long)K, (long long)G);
    OWL_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && C < (1ll << 31) - 1, "owl_map_match: need 0 < B <= 65535 and 0 < C < 2^31 - 1 (B=%lld C=%lld)", (long long)B, (long long)C);
    OWL_CHECK_ARG(det_boxes && det_scores && det_labels && det_counts && gt_boxes && gt_labels && gt_counts && scale && iou_thr && area_rng && rec_score && rec_label && rec_rank && rec_mask && npig, "owl_map_match: null pointer");
    hipLaunchKernelGGL(map_match_kernel, dim3((unsigned)(C + 1), (unsigned)B), dim3(64), 0, (hipStream_t)stream, det_boxes, det_scores, det_labels, det_counts,
                       gt_boxes, gt_labels, gt_counts, scale, iou_thr, area_rng, rec_score, rec_label, rec_rank, rec_mask, npig, (int)K, (int)G, (int)C);
    OWL_LAUNCH_CHECK();
    return 0;
}

OWL_API int owl_map_accumulate(void* stream, const int* rec_rank, const int* rec_mask, const int64_t* seg, const int* npig, const double* rec_thr,
                               const int* max_dets, double eps, double* precision, double* recall, int64_t N, int64_t C) {
    OWL_CHECK_ARG(N >= 0 && C > 0 && C <= 65535, "owl_map_accumulate: need N >= 0 and 0 < C <= 65535 (N=%lld C=%lld)", (long long)N, (long long)C);
    OWL_CHECK_ARG((N == 0 || (rec_rank && rec_mask)) && seg && npig && rec_thr && max_dets && precision && recall, "owl_map_accumulate: null pointer");
    hipLaunchKernelGGL(map_accumulate_kernel, dim3(MAP_A * MAP_M * MAP_T, (unsigned)C), dim3(64), 0, (hipStream_t)stream, rec_rank, rec_mask, seg, npig, rec_thr,
                       max_dets, eps, precision, recall, (int)C);
    OWL_LAUNCH_CHECK();
    return 0;
}
