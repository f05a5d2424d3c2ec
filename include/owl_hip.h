/*
 * libowlhip -- C ABI of the MI355X-native OWL-ViT train path (gfx950 / CDNA4).
 *
 * The reference (stevebottos/owl-vit-object-detection) has NO native layer: its hot path is Python
 * over stock aten kernels.  The drop-in boundary is therefore the Python
 * call surface (`model(image)`, `PushPullLoss(...)`, `HungarianMatcher(...)`; for the open-vocabulary
 * path `model.forward_queries(...)`, `OpenVocabLoss(...)`, `OpenVocabMatcher(...)`, whose contract is
 * transformers' Deformable-DETR criterion, `TF:` = transformers/loss/loss_deformable_detr.py); this
 * header is the thin C ABI underneath it.  Each entry point names the reference arithmetic it replaces
 * (`ref:` = path under the reference repo, `HF5:` = transformers/models/owlvit/modeling_owlvit.py).
 *
 * Conventions:
 *   - every function enqueues on the hipStream_t passed as `stream` and returns immediately;
 *     0 = OK, <0 = error (message via owl_last_error(), thread-local);
 *   - re-entrant: the library keeps NO process-global mutable state (kernel choices are per-call arguments; the tuning
 *     switches of tools/ exist only in an OWL_TUNING build, include/owl_hip_tuning.h);
 *   - ops that need device scratch take it from the caller (`*_workspace_bytes` / `*_workspace` queries size it);
 *   - the library never allocates or frees device memory; all pointers are device pointers to
 *     contiguous row-major buffers owned by the caller; outputs are pre-allocated;
 *   - bf16 buffers are passed as `void*` (raw 16-bit words), f32 as `float*`;
 *   - activations are laid out [B * Tp, width] with Tp = tokens padded to a multiple of 8 per
 *     image (class token first); allocations are padded to a multiple of 128 rows.
 *
 * The prototypes below are parsed by owl_vit_object_detection_amd/_lib.py to build the ctypes
 * signatures -- keep one prototype per statement, plain C types only.
 */
#ifndef OWL_HIP_H
#define OWL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ---------------------------------------------------------------------------------- */
/* Bumped whenever a prototype, an argument's meaning or a caller-provided scratch layout changes (1 = round 1; 2 = round 2: per-call `tile` /
 * `variant` arguments, partial-sum scratch of the row reductions, 5D+4 box_final_bwd partials; 3 = round 3; 4 = round 4: `slow_tiles` statistic of the attention forward; 5 = round 5: owl_patch_embed_bf16's weight layout for patch sizes that are not 2^n (gathered, no im2row); the V^T attention form, attention variants 3-5, GEMM epilogues 5 / 6 and tiles 8 / 9 / 5 / 4 moved to OWL_TUNING builds); 6 = round 6: + owl_patch_embed_scratch_bytes, owl_normalize_u8, owl_allreduce_sum_f32, `phases` of owl_attention_bwd_bf16; GEMM epilogue 1 saves quick_gelu'(u) and epilogue 8 multiplies by it; patch sizes must be even; 7: + owl_map_match, owl_map_accumulate (COCO bbox mAP of the eval loop); 8: + the wide class head for label sets beyond 10 classes (owl_query_normalize_wide, owl_class_sims_wide_fwd, owl_class_sims_wide_bwd, owl_query_normalize_wide_bwd); still 8: + owl_grad_norm_workspace_bytes, owl_grad_sumsq, owl_adamw_step_grouped (clipped AdamW with parameter groups) -- purely additive: no existing prototype, layout or meaning changes, so the number stays; still 8, additive again: + owl_embed_bwd, owl_im2row_bf16, owl_slab_reduce_rows (the backward below encoder layer 0, for trainable embeddings); still 8, additive again: + owl_bicubic_coeffs_box, owl_preprocess_u8_tiles (train-time crop / flip / mosaic in the device resampler); still 8, additive again: + owl_pos_resample, owl_pos_resample_bwd (the position table at another input size than the checkpoint's); still 8, additive again: + owl_gemm_nt_plan and the OWL_GEMM_KERNEL_* ids (which kernels a GEMM call launches; host query); still 8, additive again: + owl_prefix_emit, owl_prefix_gather (the frozen-prefix activation cache); still 8, additive again: + owl_image_query_workspace_bytes, owl_image_query_select, owl_query_bank_fill (the query bank from image exemplars); still 8, additive again: + owl_focal_match_cost, owl_focal_loss_workspace_bytes, owl_focal_loss_fwd, owl_box_pair_loss, owl_open_vocab_loss_reduce, owl_focal_loss_bwd, owl_box_pair_loss_bwd (the open-vocabulary criterion over [B, P, Q] logits); still 8, additive again: + owl_box_rows_compact_blocks, owl_box_rows_compact, owl_box_rows_gather, owl_box_rows_put, owl_box_rows_scatter_add (the box head's dX GEMMs on the rows that carry a gradient).  owl_abi_version() returns the value
 * the library was BUILT with: a binding compares it with the header it was generated from and refuses a mismatch (_lib.load() does). */
#define OWL_ABI_VERSION 8
const char* owl_last_error(void);
int owl_abi_version(void);

/* ---- GEMM  C[M,N] = A[M,K] . W[N,K]^T with fused epilogue ---------------------------------------
 * replaces aten::addmm/mm under HF5:437-439,457 (q/k/v/out proj), HF5:472,474 (fc1/fc2),
 * HF5:994-997 (box head dense0/1), ref src/models.py:25 (class dense0) and their autograd forms.
 * epi: 0 bias->bf16 | 1 bias+quick_gelu->bf16 (aux, optional = bf16 quick_gelu'(pre-activation): ABI 6; ABI <= 5 saved the pre-activation) |
 *      2 bias+erf-gelu->bf16 (aux, optional = pre-activation) |
 *      3 resid+acc+bias->f32 | 4 alpha*acc(+bias)->f32 | 8 acc*aux->bf16 (aux = what epi 1 saved: the dX GEMM through quick-GELU is one multiply, ABI 6) |
 *      9 acc*gelu'(aux)->bf16 | 10 out f32 += acc | 11 split-K slab
 *      (5 atomicAdd f32 and 6 per-head transposed bf16: OWL_TUNING builds only -- the train path uses neither).
 * a_rows / w_rows clamp the tile loads; M, N guard the stores; K % 64 == 0.
 * tile: kernel choice, per call (no global state): 0 = automatic (large shapes: 256x256x64 tiles on the two-phase ping-pong schedule, 8 waves,
 *       gemm_pp2.hip -- for narrow outputs with the remainder round on half-height 128x256 tiles, gemm_pph.hip --; 128x128x64 otherwise); tests pin one
 *       kernel with 128 | 256 (the single-phase REFERENCE kernel every other one is held to, bit for bit) | 7 (two-phase ping-pong on the whole
 *       problem) | 6 (= 0, plus: a problem of at most 128 tiles of 256 x 256 -- half a round of the 256 CUs -- runs every tile as two half-height tiles;
 *       for callers that know nothing else is in flight: batch 1 / 2, one stream).  All give identical bits.  (8, 9, 5, 4: the round-1 four-phase ping-pong, the round-4 free-running and the four-wave experiments,
 *       OWL_TUNING builds only.)                                                                                                                   */
int owl_gemm_nt_bf16(void* stream, int epi, const void* A, int64_t lda, int64_t a_rows, const void* W, int64_t ldw, int64_t w_rows, const float* bias, void* out, int64_t ldo, const float* resid, void* aux, int64_t ld_aux, int64_t M, int64_t N, int64_t K, float alpha, int splits, int64_t Tp, int tile);
/* Which kernels the call above launches, asked without a device (host function; it runs the launch's own argument checks and its own planner):
 * returns the number of steps, 1 or 2, with kernels[i] = OWL_GEMM_KERNEL_* and rows[i] = the rows of M that step computes (two steps: rows
 * [0, rows[0]) on kernels[0], the rest on kernels[1]); <0 with owl_last_error() for arguments the launch refuses.  has_aux: would `aux` be
 * non-NULL.  `kernels`, `rows`: HOST arrays of 2. */
#define OWL_GEMM_KERNEL_SP128 0   /* single-phase 128 x 128 (gemm.hip) */
#define OWL_GEMM_KERNEL_SP256 1   /* single-phase 256 x 256 (gemm.hip) */
#define OWL_GEMM_KERNEL_PP2 2     /* two-phase ping-pong 256 x 256 (gemm_pp2.hip) */
#define OWL_GEMM_KERNEL_PPH 3     /* half-height ping-pong 128 x 256 (gemm_pph.hip) */
int owl_gemm_nt_plan(int epi, int64_t M, int64_t N, int64_t K, int64_t a_rows, int has_aux, int64_t Tp, int splits, int tile, int* kernels, int64_t* rows);
/* epi 11 = split-K partial slabs out[split][M][ldo] (f32, no atomics); reduce them with owl_slab_reduce */
int owl_gemm_effective_splits(int64_t K, int splits);
/* f32 slab scratch of an epi-11 call (M, N, K, splits): bytes = owl_gemm_effective_splits(K, splits) * M * ldo * 4 (`bytes`: HOST pointer) */
int owl_gemm_slab_workspace_bytes(int64_t M, int64_t ldo, int64_t K, int splits, int64_t* bytes);
int owl_slab_reduce(void* stream, const float* slabs, float* out, int64_t n, int64_t slab_stride, int nsplit, int accumulate);

/* ---- patch embedding (HF5:282-288 Conv2d k=s=patch, no bias; HF5:336-343 flatten + positions) ----
 * im2row-free for EVERY even patch size 8 <= ps <= 64: the A-operand loader gathers 16-byte runs of each patch row straight from the
 * bf16 image [B,3,S,S] into LDS.  x_out[b*Tp + 1 + p, :] = W_pe . vec(patch) + pos[1+p, :].
 *   ps = 2^n      : w_pe = the conv weight [D, 3*ps*ps] as it lies.
 *   other ps (14) : the K index pads a patch row to psp = 2^n >= ps positions; position `pos` of a row holds pixel
 *                   min(8*(pos/8), ps - 8) + pos%8 -- the last 16-byte chunk of a row OVERLAPS its predecessor instead of leaving the
 *                   patch -- and w_pe is [D, Kg], Kg = 3*ps*psp rounded up to 64, with the conv weight at each pixel's FIRST position
 *                   and zeros elsewhere (Python: weights.patch_weight_gather_layout).  (ABI 5; ABI <= 4 took an explicit im2row there.)
 * scratch: bf16 [rows128(B*P), Kg], needed only when a single-phase reference kernel (tile 256 / 128, or a problem too small for the
 *          ping-pong kernel) meets a patch size that is not 2^n (explicit im2row in the same K order: identical bits); else NULL.
 *          owl_patch_embed_scratch_bytes answers "how many bytes, for this problem and tile" (0 = pass NULL): the dispatcher's rule lives there only (ABI 6).
 * tile: 0 = automatic (two-phase ping-pong kernel for big problems), 7 / 256 / 128 pin a kernel (tests); same bits.       */
int owl_patch_embed_scratch_bytes(int64_t B, int64_t S, int64_t ps, int64_t D, int tile, int64_t* bytes);
int owl_patch_embed_bf16(void* stream, const void* image_bf16, const void* w_pe, const float* pos, float* x_out, void* scratch, int64_t B, int64_t S, int64_t ps, int64_t D, int64_t Tp, int tile);
/* Rectangular images (still ABI 8: additive).  image bf16 [B, 3, H, W]; gh = H / ps, gw = W / ps; patch p = y * gw + x (the order of conv2d(...).flatten(2))
 * goes to row b * Tp + 1 + p.  The same kernels as the square entries, which ARE these with H = W = S (same bits): the gather's row stride and patch-row
 * divisor are W and gw, its channel stride H * W.  Refused before any launch: H or W no multiple of ps; ps odd or outside 8 .. 64 (W is then even, which the
 * 16-byte LDS-DMA pieces need); Tp < gh * gw + 1; B * 3 * H * W * 2 >= 2^32 or B * gh * gw >= 2^31 (32-bit gather offsets).                                */
int owl_patch_embed_scratch_bytes_hw(int64_t B, int64_t H, int64_t W, int64_t ps, int64_t D, int tile, int64_t* bytes);
int owl_patch_embed_bf16_hw(void* stream, const void* image_bf16, const void* w_pe, const float* pos, float* x_out, void* scratch, int64_t B, int64_t H, int64_t W, int64_t ps, int64_t D, int64_t Tp, int tile);
/* class-token rows x[b*Tp, :] = class_embedding + pos[0, :]  (HF5:338-343)                        */
int owl_cls_rows(void* stream, float* x, const float* cls, const float* pos, int64_t B, int64_t Tp, int64_t D);
/* Position table at another input size than the checkpoint's (HF5:296-332 `interpolate_pos_encoding`; still ABI 8: additive).  pos f32 [g0 g0 + 1, D] is
 * the native table (row 0 the class token, then the g0 x g0 patch rows, row-major), out f32 [g g + 1, D] the table the embeddings above are handed:
 *   out[0] = pos[0];   out[1 + y g + x] = sum_{i, j < 4} wy_i wx_j pos[1 + cy_i g0 + cx_j]
 * = torch.nn.functional.interpolate(mode="bicubic", align_corners=False, size=(g, g)) on the patch rows.  Per axis: source coordinate
 * s = (o + 0.5) g0 / g - 0.5, f = floor(s), t = s - f (formed in integers: one f32 rounding); taps f - 1 .. f + 2 CLAMPED to [0, g0 - 1] (clamped taps add up
 * on the border cell); cubic-convolution weights with A = -0.75: w0 = c2(t + 1), w1 = c1(t), w2 = c1(1 - t), w3 = c2(2 - t),
 * c1(x) = ((A + 2) x - (A + 3)) x x + 1, c2(x) = ((A x - 5 A) x + 8 A) x - 4 A.  No antialiasing when shrinking.  g == g0 gives weights {0, 1, 0, 0}: a copy.
 * owl_pos_resample_bwd is the exact adjoint and ACCUMULATES like every gradient entry: dpos[0] += dU[0], dpos[1 + c] += sum over the output cells whose
 * clamped taps touch source cell c, walked in ascending (y, x) order by the one thread that owns (c, 4 columns): a gather, no atomics, bitwise reproducible.
 * 1 <= g0, g <= 256 (g0 < 4: every tap clamped); D % 8 == 0; rows 16-byte aligned.  One launch each, no scratch.                                        */
int owl_pos_resample(void* stream, const float* pos, float* out, int64_t g0, int64_t g, int64_t D);
int owl_pos_resample_bwd(void* stream, const float* dU, float* dpos, int64_t g0, int64_t g, int64_t D);
/* The same pair onto a rectangular run grid (still ABI 8: additive): the native table stays [g0 g0 + 1, D], the run table is [gh gw + 1, D] with row
 * 1 + y gw + x; the y axis takes its taps with gh, the x axis with gw (HF's interpolate(size=(gh, gw))).  Same kernels, evaluation order and fmaf count; the
 * square entries are these with gh = gw = g.  1 <= g0, gh, gw <= 256.                                                                                       */
int owl_pos_resample_hw(void* stream, const float* pos, float* out, int64_t g0, int64_t gh, int64_t gw, int64_t D);
int owl_pos_resample_bwd_hw(void* stream, const float* dU, float* dpos, int64_t g0, int64_t gh, int64_t gw, int64_t D);

/* ---- LayerNorm (HF5:484-486, 721-723; eps 1e-5).  out bf16 or f32 (may alias x); stats = (mean,rstd) */
int owl_layernorm_fwd(void* stream, const float* x, const float* gamma, const float* beta, void* out, int out_bf16, float* stats, int64_t rows, int64_t D, float eps);
/* fused residual add: x_out = x + delta (bf16 output of the previous branch's GEMM, HF5:500,507 `residual + hidden_states`),
 * out = LN(x_out).  x_out may alias x.                                                                              */
int owl_add_layernorm_fwd(void* stream, const float* x, const void* delta_bf16, float* x_out, const float* gamma, const float* beta, void* out, int out_bf16, float* stats, int64_t rows, int64_t D, float eps, const void* delta2_bf16);

/* ---- fused self-attention forward (HF5:377-402): softmax(Q K^T * scale) V, dh = 64 -----------------
 * q, k, v row-major [B*Tp, ld_qkv] (head h at column h*64 of each; normally three column slices of the one [B*Tp, 3D] QKV GEMM output,
 * HF5:437-439); out row-major [B*Tp, ld_out]; lse optional [B,H,Tp] (log2 domain).  V is read where the QKV GEMM leaves it: the
 * [64 key][64 d] tile is transposed by the LDS hardware (ds_read_b64_tr_b16) -- no V^T copy of anything exists.
 * variant (per call, no global state): 0 = the library's choice; 1 = plain tiling (tokens 0..T-1 in 64-key tiles / 128-query blocks);
 * 2 = class token peeled: token 0 enters every other query's online softmax as its initial state and is itself one VALU-only workgroup
 * per (image, head), the tiles cover tokens 1..T-1 -- needs T - 1 a positive multiple of 64 (else rc != 0); same values as 1 to bf16
 * round-off (other summation order), 5.8 % faster at T = 2305.  0 picks 2 wherever it is allowed.
 * slow_tiles (optional, may be NULL): device int, += 1 for every (wave = 32 queries, 64-key tile) pair that leaves the fast path -- the tile's row sums
 * against the offset the wave already holds exceed 2^40 (or are inf / NaN) and the tile is recomputed with an explicit maximum.  A wave's first tile
 * is not counted.  Zero on scores of ordinary size (HF-init weights); trained-like weights with attention sinks trip it about once per wave and layer.
 * (The round-1 V^T form, the one-wave-per-SIMD and the 12-wave experiments: OWL_TUNING builds, include/owl_hip_tuning.h.) */
int owl_attention_fwd_vrow_bf16(void* stream, const void* q, const void* k, const void* v, int64_t ld_qkv, void* out, int64_t ld_out, float* lse, int64_t B, int64_t H, int64_t T, int64_t Tp, float scale, int variant, int* slow_tiles);

/* backward of the fused attention (layers whose attention runs backward): qkv row-major [B*Tp,3D] (q|k|v), dO / O row-major
 * [B*Tp,D], lse from the forward; writes dqkv [B*Tp,3D] (dq|dk|dv, bf16).  Every transposed operand of the dK/dV/dQ MFMAs is read
 * out of the row-major tiles by the LDS hardware (ds_read_b64_tr_b16): no Q^T / K^T / dO^T copies exist.  dvec_ws: f32 [B,H,Tp]. */
int owl_attention_bwd_workspace_bytes(int64_t B, int64_t H, int64_t Tp, int64_t* bytes);   /* dvec_ws; `bytes` is a HOST pointer */
int owl_attention_bwd_bf16(void* stream, const void* qkv, const void* dO, const void* O, const float* lse, float* dvec_ws, void* dqkv, int64_t B, int64_t H, int64_t T, int64_t Tp, float scale, int phases);   /* phases (ABI 6): 0 = all three kernels; else a mask 1 dvec | 2 dK, dV | 4 dQ -- the last two only share inputs and may go to two streams behind the first */

/* ---- post_layernorm on all tokens + class-token merge + post_post_layernorm (ref src/models.py:80-86);
 * optional fused final residual add (delta_bf16 -> x_out = x + delta, may alias x)                      */
int owl_merge_ln_fwd(void* stream, const float* x, const void* delta_bf16, float* x_out, const float* g1, const float* b1, const float* g2, const float* b2, float* cls_ln, void* feats_bf16, float* stats1, float* stats2, int64_t B, int64_t P, int64_t Tp, int64_t D, float eps);

/* ---- heads -------------------------------------------------------------------------------------- */
/* qhat = Q/|Q| + 1e-6 (ref src/models.py:31-33, eps placement literal); padded to 32 rows        */
int owl_query_normalize(void* stream, const float* queries, float* qhat32, float* qnorm, int64_t nq, int64_t Dt);
/* sims = max over 3 prompts of (e/(|e|+1e-6)) . qhat (ref src/models.py:25-36); f32 MFMA            */
int owl_class_sims_fwd(void* stream, const float* e, const float* qhat32, float* sims, unsigned char* argmax, float* inv_norm, int64_t rows, int64_t Dt, int64_t C);
/* Wide class head (ABI 8): label sets of 1 <= C <= 384 classes; the model takes it for 3C > 32, the entries above keep their 32-prompt limit.
 * qhat_wide is [nblk][32][Dt] f32 with nblk = ceil(C / 10): class c in block c / 10, its prompts in rows 3 (c % 10) .. + 2, rows 30 / 31 and the
 * rows of classes >= C zero; qnorm (optional) [32 nblk].  nq = 3 C.                                                                          */
int owl_query_normalize_wide(void* stream, const float* queries, float* qhat_wide, float* qnorm, int64_t nq, int64_t Dt);
/* sims [rows, C] f32, argmax [rows, C] u8, inv_norm [rows]: column c carries the bits owl_class_sims_fwd gives for a call on classes
 * 10 (c / 10) .. + 9 alone.  Dt % 64 == 0                                                                                                   */
int owl_class_sims_wide_fwd(void* stream, const float* e, const float* qhat_wide, float* sims, unsigned char* argmax, float* inv_norm, int64_t rows, int64_t Dt, int64_t C);
/* dense2 + box bias + sigmoid + center_to_corners (HF5:998, 1071-1104; ref src/models.py:70-73); D % 8 == 0, D <= 1024 */
int owl_box_final_fwd(void* stream, const void* h_bf16, const float* w2, const float* b2, const float* box_bias, float* boxes, float* sig_out, int64_t rows, int64_t P, int64_t D);

/* ---- Hungarian-matched push-pull loss, fully on device (no host sync) --------------------------------
 * Targets are padded: labels [B,Nmax] i64, tgt_boxes [B,Nmax,4] f32, counts [B] i32.
 * costT[b][j][p] = w_bbox*|box_p - tgt_j|_1 - w_class*softmax(sims_p)[label_j] - w_giou*GIoU   (ref src/matcher.py:106-131).
 * A label outside [0, C) never indexes sims: its class term is 0 and owl_push_pull_loss returns loss_ce = NaN for that batch
 * (the reference raises IndexError / one_hot error; validate on the host where the labels are host tensors). */
/* ragged per-image target lists (ref main.py:77-79; src/matcher.py:94-104 `targets`) -> the padded form in ONE launch: labels_cat i64 [N],
 * boxes_cat f32 [N,4] = the lists concatenated in image order, offsets i32 [B+1] (device) = image boundaries; pads are zero-filled. */
int owl_pack_targets(void* stream, const int64_t* labels_cat, const float* boxes_cat, const int* offsets, int64_t* labels, float* boxes, int* counts, int64_t B, int64_t Nmax);
int owl_match_cost(void* stream, const float* sims, const float* boxes, const int64_t* labels, const float* tgt_boxes, const int* counts, float* costT, int64_t B, int64_t P, int64_t C, int64_t Nmax, float w_class, float w_bbox, float w_giou);
/* rectangular LSAP per image (replaces scipy.optimize.linear_sum_assignment at ref src/matcher.py:134-137, f64 duals,
 * scipy's tie rule) + target scatter (ref src/matcher.py:146-157): pairs ordered by prediction index             */
int owl_hungarian(void* stream, const float* costT, const int64_t* labels, const int* counts, int64_t* pred_idx, int64_t* tgt_idx, int64_t* target_classes, int64_t B, int64_t P, int64_t Nmax, int64_t bg);
/* sequential IoU > thr label spreading (ref src/losses.py:100-106), in place on target_classes [B,P]             */
int owl_spread_labels(void* stream, const float* boxes, int64_t* target_classes, int64_t B, int64_t P, int64_t bg, float thr);
/* class_loss (ref src/losses.py:16-40) + loss_boxes (ref src/losses.py:42-69); losses[4] = mean over images of
 * {loss_ce, loss_bg, loss_bbox, loss_giou}; optional per-term gradients wrt sims / boxes                          */
int owl_push_pull_loss(void* stream, const float* sims, const float* boxes, const int64_t* target_classes, const float* scales, const float* tgt_boxes, const int64_t* pred_idx, const int64_t* tgt_idx, const int* counts, float* per_image, float* losses, float* dsims, float* dl1, float* dgiou, int64_t B, int64_t P, int64_t C, int64_t Nmax, int64_t bg);
int owl_push_pull_loss_bwd(void* stream, const float* g4, const int64_t* target_classes, const float* dsims, const float* dl1, const float* dgiou, float* out_sims, float* out_boxes, int64_t B, int64_t P, int64_t C, int64_t bg);

/* ---- inference post-process, fully on device (ref src/models.py:122-146 PostProcess.__call__; top-k prefix = ref
 * main.py:114-117).  Per image: score = max_c sims, class = first arg-max, keep score > conf_thr, class-aware NMS
 * (torchvision.ops.batched_nms semantics: same class, IoU > iou_thr, lower score suppressed), results ordered by
 * descending score (ties: ascending patch index), at most max_out per image.
 * route: which of torchvision's two batched_nms routes -- 0 per class on the raw coordinates (_batched_nms_vanilla), 1 coordinate
 * offset boxes + class * (max + 1) then one class-agnostic NMS (_batched_nms_coordinate_trick), 2 / 3 torchvision's own choice for a
 * GPU / CPU tensor (coordinate trick up to 20 000 / 4 000 coordinates past the threshold).  They differ only where the f32 rounding of
 * the shifted coordinates moves an IoU across the threshold.
 * The selection follows torch.max: a row with a NaN in any column is dropped, -0.0 == +0.0 (score ties: lower patch index first), and
 * out_scores holds the winning column's own bits.
 * boxes [B,P,4] f32 xyxy, sims [B,P,C] f32 -> out_boxes [B,max_out,4], out_scores [B,max_out], out_classes [B,max_out] i64,
 * out_patch [B,max_out] i64 (source patch index), out_count [B] i32; entries beyond the count are left untouched.
 * workspace: device scratch of owl_postprocess_workspace() bytes (16-byte aligned); `bytes` is a HOST pointer.     */
int owl_postprocess_workspace(int64_t B, int64_t P, int64_t* bytes);
int owl_postprocess(void* stream, const float* boxes, const float* sims, void* workspace, int64_t ws_bytes, float* out_boxes, float* out_scores, int64_t* out_classes, int64_t* out_patch, int* out_count, int64_t B, int64_t P, int64_t C, int64_t max_out, float conf_thr, float iou_thr, int route);

/* ---- sliced inference, the merge (csrc/slice_merge.hip): the candidates owl_postprocess left on T slices become one detection list per source image.
 * boxes [T,K,4] f32, scores [T,K] f32, classes [T,K] i64, counts [T] i32 are owl_postprocess' outputs on the slices (slots past a slice's count are never
 * read); xform [T,4] f32 rows (sx, ox, sy, oy) map a slice's box into its source image: x = ox + bx * sx, y = oy + by * sy (an f32 multiply, then an f32 add;
 * no clipping); slice_offsets [G+1] i32 is a CSR over the G source images (device arrays, both).  Candidate c = local_slice * K + rank of a source image is
 * live iff rank < counts[slice] and its score is not NaN; order: score descending, then c ascending, -0.0 == +0.0; out_scores keeps the input's bits.
 * Greedy suppression of the lower-ranked candidate where the classes are equal (class_aware 1; any pair with 0) and ovr > thr; metric 0: ovr = inter /
 * (ai + aj - inter), owl_postprocess' per-class route operation for operation; metric 1: ovr = inter / min(ai, aj) (intersection over the smaller area:
 * a box cut by a slice border against the whole box from the neighbouring slice).  0 / 0 is NaN and suppresses nothing.  At most max_out per source image.
 * Nmax >= K times the largest slice count of a group, <= 8192.  -> out_boxes [G,max_out,4] (full-image coordinates), out_scores [G,max_out], out_classes
 * [G,max_out] i64, out_src [G,max_out] i64 (= c: c / K is the slice within the group, c % K the rank in it), out_count [G] i32; entries beyond the count
 * are left untouched.  Three launches, no host sync.  workspace: owl_slice_merge_workspace() bytes of device scratch (16-byte aligned); `bytes` is a HOST
 * pointer.  boxes, xform and out_boxes are 16-byte aligned.  Additive: the ABI version is unchanged.                                                       */
int owl_slice_merge_workspace(int64_t G, int64_t Nmax, int64_t* bytes);
int owl_slice_merge(void* stream, const float* boxes, const float* scores, const int64_t* classes, const int* counts, const float* xform, const int* slice_offsets, void* workspace, int64_t ws_bytes, float* out_boxes, float* out_scores, int64_t* out_classes, int64_t* out_src, int* out_count, int64_t T, int64_t K, int64_t G, int64_t Nmax, int64_t max_out, float thr, int metric, int class_aware);

/* ---- COCO bbox mAP of the eval loop, on device (ref main.py:31,120-128,144-147; src/train_util.py:37-64 -> torchmetrics
 * MeanAveragePrecision(iou_type="bbox", class_metrics=True) -> the pycocotools COCOeval protocol evaluateImg / accumulate).  ABI 7.
 * The protocol's constants come from the caller as device arrays and are never re-derived in device code: iou_thr f64 [10] (linspace(0.5, 0.95, 10)),
 * area_rng f64 [4][2] = {lo, hi} of all / small / medium / large, rec_thr f64 [101] (linspace(0, 1, 101)), max_dets i32 [3] = {1, 10, 100}, eps = spacing(1).
 * The counts 10 / 4 / 3 / 101 and the cut to 100 detections per (image, class) are part of the record layout.
 * owl_map_match -- one launch per metric update, no host sync.  det_boxes [B,K,4] f32 xyxy, det_scores [B,K], det_labels [B,K] i64, det_counts [B] i32 (slots
 * past the count and labels outside [0, C) are padding: the batched PostProcess layout pads with -1); gt_boxes [B,G,4], gt_labels [B,G] i64, gt_counts [B];
 * scale [B,2] f32 = (sx, sy) multiplied onto x / y of both box sets in f32 (1 for pixel boxes, width / height for normalised ones, ref src/util.py:94-97).
 * Detections need not be sorted: the kernel ranks the detections of an (image, class) by descending score, ties by slot, and keeps 100.
 * Per detection slot: rec_score [B,K] f32, rec_label [B,K] i64 (-1: the slot is no record -- padding, label out of range, rank >= 100), rec_rank [B,K] i32
 * (rank within its image and class), rec_mask [B,K,4] i32, one word per area range: bit t = matched at IoU threshold t, bit 10 + t = ignored at t.
 * npig [B,C,4] i32 = ground truths of the class inside the area range.  K <= 1024, G <= 256.
 * owl_map_accumulate -- one launch per compute().  rec_rank [N] / rec_mask [N,4]: the records of all updates, ordered by class, inside a class by descending
 * score, stable in arrival order; seg i64 [C+1] = class boundaries in that order; npig i32 [C,4] summed over the images.
 * -> precision f64 [10,101,C,4,3], recall f64 [10,C,4,3]; -1 where a (class, area range) has no ground truth.  No scratch. */
int owl_map_match(void* stream, const float* det_boxes, const float* det_scores, const int64_t* det_labels, const int* det_counts, const float* gt_boxes, const int64_t* gt_labels, const int* gt_counts, const float* scale, const double* iou_thr, const double* area_rng, float* rec_score, int64_t* rec_label, int* rec_rank, int* rec_mask, int* npig, int64_t B, int64_t K, int64_t G, int64_t C);
int owl_map_accumulate(void* stream, const int* rec_rank, const int* rec_mask, const int64_t* seg, const int* npig, const double* rec_thr, const int* max_dets, double eps, double* precision, double* recall, int64_t N, int64_t C);

/* ---- the one collective of the path: in-place SUM of the flat f32 gradient bucket over the data-parallel ranks on `stream`, through the
 * CALLER's RCCL communicator (`rccl_comm` = an `ncclComm_t`).  For hosts without PyTorch; this repo's Python host issues the same collective through
 * torch.distributed (torch owns its communicator).  librccl.so is bound lazily at the first call: no load-time dependency.  Scale by 1 / world in
 * owl_adamw_step (`grad_scale`).  ABI 6.                                                                                                                          */
int owl_allreduce_sum_f32(void* stream, void* rccl_comm, float* buf, int64_t n);

/* ---- device input pipeline (ref src/dataset.py:69-71: HF OwlViTImageProcessor = PIL bicubic resize -> x(1/255) ->
 * (x-mean)/std).  owl_bicubic_coeffs is HOST-side (all pointers host): Pillow's Resample.c tap tables for one axis,
 * bounds[2*out] = {first tap, tap count}, kk[out*ksize] 22-bit fixed point; kk_capacity in ints; ksize returned.
 * owl_preprocess_u8_batch (device pointers), per image: src RGB u8 [H,W,3] -> horizontal pass into tmp u8 [H,out_w,3] -> vertical pass
 * -> lut[3][256] (the reference's rescale+normalize value of each u8 level) -> out [3,out_h,out_w] f32 or bf16.      */
int owl_bicubic_coeffs(int64_t in_size, int64_t out_size, int* bounds, int* kk, int64_t kk_capacity, int* ksize_out);
/* one launch pair for a ragged batch: desc = n_images x 10 int64 in DEVICE memory, per image
 * {src ptr, H, W, bounds_x ptr, kk_x ptr, ksize_x, bounds_y ptr, kk_y ptr, ksize_y, byte offset of its intermediate in tmp};
 * out [n_images,3,out_h,out_w]                                                                                        */
int owl_preprocess_u8_batch(void* stream, const void* desc, int64_t n_images, int64_t max_h, unsigned char* tmp, const float* lut, void* out, int out_bf16, int64_t out_h, int64_t out_w);
/* Train-time augmentation in the resampler (ABI 8, additive).  owl_bicubic_coeffs_box (HOST pointers): owl_bicubic_coeffs for the source box [in0, in1) of the axis
 * (0 <= in0 < in1 <= in_size, float edges) = Pillow's precompute_coeffs under Image.resize(size, BICUBIC, box=...): scale = (in1 - in0) / out_size,
 * center = in0 + (xx + 0.5) * scale, taps clipped to [0, in_size) (the image, not the box).  in0 = 0, in1 = in_size gives the bits of owl_bicubic_coeffs.  */
int owl_bicubic_coeffs_box(int64_t in_size, double in0, double in1, int64_t out_size, int* bounds, int* kk, int64_t kk_capacity, int* ksize_out);
/* owl_preprocess_u8_tiles (device pointers): one launch pair for a list of TILES, each one resample source box -> a cw x ch cell of output image b:
 * desc = n_tiles x 18 int64 in DEVICE memory, per tile {src ptr, H, W, bounds_x ptr, kk_x ptr, ksize_x (tables of cw entries), bounds_y ptr, kk_y ptr,
 * ksize_y (ch entries), y_first, n_rows (the source rows the vertical taps read: bounds_y[0] .. bounds_y[2ch-2] + bounds_y[2ch-1]), byte offset of its
 * u8 [n_rows,cw,3] intermediate in tmp, b, x0, y0, cw, ch, flip}; writes out[b, :, y0 + y, x0 + (flip ? cw - 1 - x : x)] = lut[c][level], out
 * [n_out,3,out_h,out_w] f32 | bf16.  max_rows = max n_rows.  The CALLER guarantees 0 <= b < n_out and that the cells of every output image lie inside it
 * and cover it exactly (the descriptors live in device memory: preprocess.check_tile_cover is the host check).                                          */
int owl_preprocess_u8_tiles(void* stream, const void* desc, int64_t n_tiles, int64_t max_rows, unsigned char* tmp, const float* lut, void* out, int out_bf16, int64_t n_out, int64_t out_h, int64_t out_w);
/* Colour jitter in the tile resampler (still ABI 8: additive; csrc/color_jitter.hip).  owl_preprocess_u8_tiles_color = owl_preprocess_u8_tiles with Pillow's
 * ImageEnhance.Brightness / Contrast / Color applied to every tile's resized cell, bit for bit, between the resize and the table:
 * color = n_tiles x 4 f32 in DEVICE memory (16-byte aligned), per tile {fb, fc, fs, order}: factors >= 0 and order 0..5 (stored as a float) indexing
 * itertools.permutations("bcs") in lexicographic order = the sequence the three ops are applied in.  Brightness(f) = blend(0, c, f), Color(f) = blend(L, c, f),
 * Contrast(f) = blend(m, c, f); L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; m = (2 sum L + n) / (2 n) over the n = cw x ch pixels of the cell as they
 * are when contrast is reached; blend(a, b, f) = clip-then-truncate of f32(a) + fl32(f * f32(b - a)) (two roundings).  A factor of exactly 1 is the identity;
 * the all-ones array gives the bits of owl_preprocess_u8_tiles.  Grayscale = fs 0.  workspace: DEVICE memory (4-byte aligned) of at least the
 * owl_preprocess_color_workspace_bytes (HOST function; `bytes` a host pointer) of the same n_tiles / out_h / out_w; it need not be initialised.  `out` is
 * used as the u8 canvas between the passes.  Same caller guarantees as owl_preprocess_u8_tiles; the CALLER validates `color` (preprocess.check_color).     */
int owl_preprocess_color_workspace_bytes(int64_t n_tiles, int64_t out_h, int64_t out_w, int64_t* bytes);
int owl_preprocess_u8_tiles_color(void* stream, const void* desc, const float* color, int64_t n_tiles, int64_t max_rows, unsigned char* tmp, void* workspace, int64_t workspace_bytes, const float* lut, void* out, int out_bf16, int64_t n_out, int64_t out_h, int64_t out_w);
/* images that already have the model's size (ABI 6): src u8 [n,H,W,3] (src_chw = 0) or [n,3,H,W] (src_chw = 1) -> lut -> out [n,3,H,W] f32 | bf16.  Pillow's resize
 * to the size an image already has is a copy, so this IS the reference pipeline for such images, bit for bit.  H*W % 4 == 0; src 4-byte, out 16-byte aligned.       */
int owl_normalize_u8(void* stream, const unsigned char* src, int src_chw, const float* lut, void* out, int out_bf16, int64_t n_images, int64_t H, int64_t W);
/* OWLv2's input stage (still ABI 8: additive; csrc/pad_resize.hip): HF Owlv2ImageProcessorPil = x(1/255), pad bottom / right to a square of side
 * S = max(H, W), scipy gaussian_filter(sigma = max(0, (S/N - 1)/2), mode "mirror"), scipy zoom(order 1, "mirror", grid_mode) to N x N, normalise.
 * owl_pad_resize_coeffs (HOST pointers), one axis of real extent `in_extent` inside a padded axis of length `padded`: row i of (bilinear rows) x (mirrored
 * Gaussian), formed in f64, restricted to the source indices below in_extent: bounds[2*i] = {first index, tap count} (0 taps: the row lies in the pad),
 * w[i*ksize + t] the weights rounded once to f32, zero padded to ksize = the largest count (returned; <= 64), wsum[i] = the f64 sum of row i's kept weights
 * rounded once.  w_capacity in floats (out_size * 64 always suffices).  padded > 16 * out_size is an error.
 * owl_preprocess_u8_pad_resize (device pointers): one launch pair for a ragged batch.  desc = n_images x 10 int64 in DEVICE memory, the layout of
 * owl_preprocess_u8_batch's: {src ptr, H, W, bounds_x ptr, w_x ptr, ksize_x, bounds_y ptr, w_y ptr, ksize_y, byte offset of its intermediate in tmp
 * (a multiple of 16)} with each bounds array followed by ONE more int, `live` = 1 + the last output index with a tap (0: none), and each weight array
 * (out * ksize floats) followed by its `wsum` (out floats).  Horizontal pass: u8 -> f32 [H, live4_x, 3] in 0..255 units (live4 = live rounded up to 4;
 * the columns past `live` are written as 0), fmaf in ascending tap order from 0; vertical pass: the same over rows, then -- pad_value != 0 only --
 * fmaf(pad255, 1 - wsum_x[j] * wsum_y[i], v) with pad255 = fl(255 * pad_value), then fmaf(v, norm[c], norm[3 + c]) (norm: 6 floats in DEVICE memory,
 * a_c = rescale / std_c and b_c = -mean_c / std_c, each formed in f64 and rounded once) -> out [n_images,3,out_h,out_w] f32 | bf16 (round to nearest
 * even).  Every element of out is written; tmp needs max over images of offset + H * live4_x * 12 bytes, need not be initialised, and nothing is read
 * from it that this call did not write.  max_h = the largest H.  tmp_f32 and out 16-byte aligned.                                                    */
int owl_pad_resize_coeffs(int64_t in_extent, int64_t padded, int64_t out_size, int* bounds, float* w, int64_t w_capacity, int* ksize_out, float* wsum);
int owl_preprocess_u8_pad_resize(void* stream, const void* desc, int64_t n_images, int64_t max_h, float* tmp_f32, const float* norm, float pad_value, void* out, int out_bf16, int64_t out_h, int64_t out_w);

/* ---- query-bank initialisation: the CLIP-style text tower run once by ref src/models.py:155-169 (HF5:603-663, 945-970).
 * Linear / LayerNorm layers reuse owl_gemm_nt_bf16 / owl_layernorm_fwd; these are the text-only pieces:
 * x[n*S+t] = tok_emb[ids[n,t]] + pos_emb[t] (f32 [N*S,W]); causal softmax attention for S <= 64, dh = 64 on
 * qkv bf16 [N*S,3W] -> out bf16 [N*S,W]; final LN of the EOS row (arg-max id) -> text_projection (f32 [Pdim,W], no bias)
 * -> L2 normalise -> out f32 [N,Pdim].                                                                               */
int owl_text_embed(void* stream, const int64_t* ids, const float* tok_emb, const float* pos_emb, float* x, int64_t N, int64_t S, int64_t W, int64_t vocab);
int owl_causal_attention_small(void* stream, const void* qkv_bf16, void* out_bf16, int64_t N, int64_t S, int64_t heads, float scale);
int owl_text_pool_project(void* stream, const float* x, const int64_t* ids, const float* gamma, const float* beta, const float* wproj, float* out, int64_t N, int64_t S, int64_t W, int64_t Pdim, float eps);

/* weight gradients without transposed copies:  slab[s][n][k] = sum_{m in split s} dY[m][n] * X[m][k]  (dW = dY^T X; both
 * operands token-major bf16 as the other kernels leave them; the transposition happens in LDS via ds_read_b64_tr_b16).
 * zero_row: >= 512 B of device zeros (source of rows m >= M); slabs [splits_used][N][K] f32 are reduced by owl_slab_reduce;
 * splits_used is a HOST pointer.  variant: 0 = the library's choice (the ping-pong schedule), 1 = single-phase kernel, 2 = ping-pong; same bits.
 * owl_colsum_bf16: colsum[c] += sum_r in[r][c] (bias gradients).                                                                   */
int owl_gemm_tn_slab_bf16(void* stream, const void* dY, int64_t ldy, const void* X, int64_t ldx, const void* zero_row, float* slab, int64_t M, int64_t N, int64_t K, int splits, int* splits_used, int variant, float* bias_slab);   /* bias_slab (ABI 6, optional): f32 [splits_used][N] receives the column sums of dY over each split's token range from the same pass (variant 0 / 2) -- the bias gradient's partial sums; add them with owl_slab_reduce(bias_slab, db, N, N, splits_used, 1) */
int owl_colsum_bf16(void* stream, const void* in_bf16, int64_t ld, float* colsum, int64_t R, int64_t C, float* partials, int64_t partials_floats);
/* f32 slab scratch of the call above for (M, N, K, splits): bytes = splits_used * N * K * 4 (`bytes` is a HOST pointer) */
int owl_gemm_tn_slab_workspace_bytes(int64_t M, int64_t N, int64_t K, int splits, int64_t* bytes);

/* pairwise out3 = {iou, union, giou} each [N,M] (free functions box_iou / generalized_box_iou, ref src/matcher.py:8-44) */
int owl_box_pairwise(void* stream, const float* boxes1, const float* boxes2, float* out3, int64_t N, int64_t M);

/* ---- backward of the row-wise pieces (autograd forms of the entries above) --------------------------
 * parameter-gradient outputs (dgamma, dbeta, dw2, db2, dqueries, colsum) ACCUMULATE into buffers the caller zeroes once per
 * step -- they are views of the flat gradient bucket.  No atomics: every workgroup writes its partial sums into `partials`
 * (caller-provided f32 scratch, `partials_floats` elements; size it once with owl_rowreduce_workspace_bytes) and a second
 * kernel adds them in a fixed order, so the bucket is bitwise reproducible run to run.                                  */
/* bytes of partial-sum scratch that serve every entry below for activations of `groups` images x `rows_per_group` rows x up
 * to C columns (C = the widest matrix reduced over rows, e.g. the MLP width for the fc1 bias gradient); HOST pointer.   */
int owl_rowreduce_workspace_bytes(int64_t groups, int64_t rows_per_group, int64_t C, int64_t* bytes);
/* dx_bf16 (optional): bf16 copy of dx, the operand of the next dX GEMM.  dx_colsum (optional, with dgamma / dbeta): += column sums of dx
 * = the bias gradient of the linear layer whose output sits at this residual position (no separate pass over the f32 dx).             */
int owl_layernorm_bwd(void* stream, const void* dy, int dy_bf16, const float* x, const float* stats, const float* gamma, const float* dres, float* dx, float* dgamma, float* dbeta, int64_t rows, int64_t D, void* dx_bf16, float* partials, int64_t partials_floats, float* dx_colsum);
int owl_merge_ln_bwd(void* stream, const float* dfeats, const float* x, const float* cls_ln, const float* stats1, const float* stats2, const float* g1, const float* b1, const float* g2, float* dx, float* dcls_ws, float* dg1, float* db1, float* dg2, float* db2, int64_t B, int64_t P, int64_t Tp, int64_t D, float* partials, int64_t partials_floats, void* dx_bf16, float* dx_colsum);
/* (owl_merge_ln_bwd: partials >= 6 D floats per 64-row block and image; dx_colsum (optional): += column sums of dx over every token of the batch,
 * class-token rows included = the bias gradient of the last encoder layer's fc2)                                                          */
/* class head backward, row-parallel part: de (bf16 [rows,Dt]), routed upstream G (bf16 [rows,32]) and a bf16 copy of e;
 * dqhat[32,Dt] = G^T e is then a split-K owl_gemm_nt_bf16, and owl_query_normalize_bwd maps it onto dqueries            */
int owl_class_sims_bwd(void* stream, const float* dsims, const float* sims, const unsigned char* argmax, const float* inv_norm, const float* e, const float* qhat32, void* de_bf16, void* g_bf16, void* e_bf16, int64_t rows, int64_t Dt, int64_t C);
int owl_query_normalize_bwd(void* stream, const float* dqhat, const float* queries, float* dqueries, int64_t nq, int64_t Dt);
/* Wide class head backward (ABI 8).  de (bf16 [rows, Dt]) = inv * (A . qhat_wide) - coef * e as an exact-f32 MFMA product, A the upstream routed to
 * each class's arg-max prompt; G (bf16 [rows, Qp], Qp = 32 ceil(C / 10) rounded up to a multiple of 256, columns in the wide layout, pad columns
 * written as zeros) = A * inv; e_bf16 = bf16(e).  dqhat_wide [Qp, Dt] = G^T e_bf16 is a weight-gradient GEMM of the caller's;
 * owl_query_normalize_wide_bwd ACCUMULATES its image under qhat = Q/|Q| + 1e-6 into dqueries [3C, Dt].  No atomics.  Dt % 32 == 0, Dt <= 1024 */
int owl_class_sims_wide_bwd(void* stream, const float* dsims, const float* sims, const unsigned char* argmax, const float* inv_norm, const float* e, const float* qhat_wide, void* de_bf16, void* g_bf16, void* e_bf16, int64_t rows, int64_t Dt, int64_t C, int64_t Qp);
int owl_query_normalize_wide_bwd(void* stream, const float* dqhat_wide, const float* queries, float* dqueries, int64_t nq, int64_t Dt);
/* dw2 [4,D] and db2 [4] must be contiguous (dw2 then db2); partials = f32 [owl_box_final_bwd_blocks(rows)][5*D+4];
 * du1_colsum (optional, [D]): += column sums of du1 = dense1's bias gradient, from the same pass */
int owl_box_final_bwd_blocks(int64_t rows);
int owl_box_final_bwd(void* stream, const float* dboxes, const float* sig, const void* h1_bf16, const void* u1_bf16, const float* w2, void* du1_bf16, float* partials, float* dw2_db2, int64_t rows, int64_t D, float* du1_colsum);
/* OWLv2's objectness head, its tail (csrc/objectness.hip; still ABI 8: additive).  HF: Owlv2BoxPredictionHead(out_dim=1) on the detached image features; the two
 * hidden layers are owl_gemm_nt_bf16 launches (epi 2 forward; epi 9 and the weight-gradient route backward).  D % 8 == 0, 8 <= D <= 1024, rows >= 1.
 * fwd: logits[r] = sum_j h[r, j] w2[j] + b2   (h bf16 [rows, D], w2 f32 [D], b2 f32 [1], logits f32 [rows]).
 * bwd: du1 = bf16(g_r w2_j gelu'(u1_rj)) (erf form), dw2_j = sum_r g_r h1_rj, db2 = sum_r g_r, du1_colsum_j = sum_r du1_rj (f32, before the bf16 rounding: dense1's
 *   bias gradient; optional).  dw2_db2: f32 [D + 4] = dw2 [D], db2, three zeros (the reducer works in quads).  partials: f32
 *   [owl_objectness_final_bwd_blocks(rows)][2 D + 4] scratch.  Every output is WRITTEN, not accumulated into; no atomics, fixed summation order. */
int owl_objectness_final_fwd(void* stream, const void* h_bf16, const float* w2, const float* b2, float* logits, int64_t rows, int64_t D);
int owl_objectness_final_bwd_blocks(int64_t rows);
int owl_objectness_final_bwd(void* stream, const float* dlogits, const void* h1_bf16, const void* u1_bf16, const float* w2, void* du1_bf16, float* partials, float* dw2_db2, int64_t rows, int64_t D, float* du1_colsum);
/* The box head's two dX GEMMs on the rows that carry a gradient (csrc/box_rows_bwd.hip; still ABI 8: additive).  The box losses read pred_boxes at the
 * matched predictions only (ref src/losses.py `src_boxes = outputs["pred_boxes"][idx]`), so dboxes f32 [rows, 4] is zero in all but at most `cap` rows, a
 * bound the host knows without a sync.  Every kernel takes the row count from device memory; the grids are sized from cap / cap_pad (a multiple of 8, >= cap).
 *   owl_box_rows_compact: row_list int32 [cap] = the indices of the rows with a component that is not == 0, ascending (NaN and inf count as non-zero,
 *     -0.0 as zero; a prefix scan, no atomics); count_flag int32 [2 + owl_box_rows_compact_blocks(rows)] = {rows listed (<= cap), 1 if MORE than cap
 *     rows were non-zero, then the compaction's own scratch}; the other kernels read its first two words.
 *   owl_box_rows_gather: dst_k bf16 [cap_pad, D] = rows row_list[i] of src_k bf16 [rows, D], zero rows at i >= count; k = 0..2 in one launch, a NULL pair is
 *     skipped.  A set overflow flag makes every listed row NaN instead: loud in everything computed from the compact operands.
 *   owl_box_rows_put: dst_k bf16 [rows, D] row row_list[i] = row i of src_k bf16 [cap, D] for i < count, or zeros where src_k is NULL; k = 0, 1 in one launch.
 *   owl_box_rows_scatter_add: dfeats f32 [rows, D] row row_list[i] += dfc f32 [cap, D] row i for i < count (distinct rows: no atomics). */
int owl_box_rows_compact_blocks(int64_t rows);
int owl_box_rows_compact(void* stream, const float* dboxes, int64_t rows, int64_t cap, int* row_list, int* count_flag);
int owl_box_rows_put(void* stream, const void* src0, const void* src1, void* dst0, void* dst1, const int* row_list, const int* count_flag, int64_t rows, int64_t cap, int64_t D);
int owl_box_rows_gather(void* stream, const void* src0, const void* src1, const void* src2, void* dst0, void* dst1, void* dst2, const int* row_list, const int* count_flag, int64_t rows, int64_t cap_pad, int64_t D);
int owl_box_rows_scatter_add(void* stream, const float* dfc, float* dfeats, const int* row_list, const int* count_flag, int64_t rows, int64_t cap, int64_t D);
int owl_transpose_colsum_bf16(void* stream, const void* in, int64_t ld_in, void* out_t, int64_t ld_out, float* colsum, int64_t R, int64_t C, float* partials, int64_t partials_floats);
int owl_colsum_f32(void* stream, const float* in, float* colsum, int64_t R, int64_t C, float* partials, int64_t partials_floats);
/* Backward below encoder layer 0 (HF5:282-288, 336-343), run only when backbone.embeddings is trainable (still ABI 8: additive).
 * owl_embed_bwd: dx f32 [B, Tp, D] = d(output of the embeddings) -> dpos [T, D] += sum_b dx[b, t, :], dcls [D] += sum_b dx[b, 0, :], and
 * dE bf16 [B (T - 1), D] = the patch rows of dx packed without the class and pad rows (the dY operand of the patch-embedding weight gradient).  One launch;
 * the sum over b runs in index order inside one thread: no atomics, bitwise reproducible.  D % 8 == 0; dpos, dcls, dE 16-byte aligned.
 * owl_im2row_bf16: image bf16 [B, 3, S, S] -> out bf16 [B (S / ps)^2, ld_out], column (c ps + i) ps + j = pixel (c, gy ps + i, gx ps + j): the conv weight's
 * own [D, 3, ps, ps] column order (NOT the gather order of owl_patch_embed_bf16), the X operand of that weight gradient.  ld_out >= 3 ps^2, ld_out % 8 == 0;
 * columns [3 ps^2, ld_out) are not written.  ps even.                                                                                                    */
int owl_embed_bwd(void* stream, const float* dx, float* dpos, float* dcls, void* dE_bf16, int64_t B, int64_t T, int64_t Tp, int64_t D);
int owl_im2row_bf16(void* stream, const void* image_bf16, void* out_bf16, int64_t ld_out, int64_t B, int64_t S, int64_t ps);
/* owl_im2row_bf16 on a rectangular image bf16 [B, 3, H, W] -> out [B (H / ps) (W / ps), ld_out], row (b gh + gy) gw + gx (still ABI 8: additive). */
int owl_im2row_bf16_hw(void* stream, const void* image_bf16, void* out_bf16, int64_t ld_out, int64_t B, int64_t H, int64_t W, int64_t ps);
/* owl_slab_reduce for slabs with pad columns: out [rows, cols] (+)= sum_s slabs[s * slab_stride + r * ld_slab + c], splits added in index order.  For a split-K
 * weight gradient whose inner size is no multiple of 8 (owl_gemm_nt_bf16 needs N % 8 == 0: the 588 columns of L/14's patch embedding run as 592).  cols, ld_slab % 4 == 0 */
int owl_slab_reduce_rows(void* stream, const float* slabs, float* out, int64_t rows, int64_t cols, int64_t ld_slab, int64_t slab_stride, int nsplit, int accumulate);

/* ---- fused AdamW on the flat trainable bucket (replaces torch.optim.AdamW.step, ref main.py:56-60,91) -----
 * decoupled weight decay, bias-corrected; g is pre-scaled by grad_scale (1/world after the sum all-reduce);
 * optionally refreshes the bf16 compute copy in the same pass                                              */
int owl_adamw_step(void* stream, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale);

/* ---- global gradient-norm clipping + parameter groups for the step above (torch.nn.utils.clip_grad_norm_, L2, + torch.optim.AdamW with several
 * param groups), in two launches on `stream`:
 *   owl_grad_sumsq          one read of g: an f64 sum of squares per workgroup into `workspace` (owl_grad_norm_workspace_bytes(n); HOST pointer
 *                           `bytes`).  The grid depends on n alone and every sum runs in a fixed order (no atomics): the same g gives the same bits.
 *   owl_adamw_step_grouped  owl_adamw_step with lr / weight_decay per SEGMENT of the bucket: seg_end / seg_lr / seg_wd are HOST arrays of nseg entries
 *                           (1 <= nseg <= 32), read by this call and passed to the kernel by value; seg_end[s] = exclusive end offset of segment s in
 *                           elements, multiples of 4, strictly increasing, seg_end[nseg-1] == n.  A null seg_lr / seg_wd means the scalar `lr` /
 *                           `weight_decay` for every segment.  max_norm > 0: every workgroup adds the partials of owl_grad_sumsq(g) in one fixed order,
 *                           norm = sqrt(sum) * |grad_scale| (the norm of the SCALED gradient), coef = min(1, max_norm / (norm + 1e-6)), the step uses
 *                           g * grad_scale * coef, and *norm_out (DEVICE f32) receives norm -- read it whenever a sync is acceptable.  max_norm <= 0:
 *                           no clipping; workspace and norm_out are neither read nor written (may be null) and coef is exactly 1.
 * One segment over everything without clipping gives the bits of owl_adamw_step.                                                                 */
int owl_grad_norm_workspace_bytes(int64_t n, int64_t* bytes);
int owl_grad_sumsq(void* stream, const float* g, int64_t n, void* workspace);
int owl_adamw_step_grouped(void* stream, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale, const int64_t* seg_end, const float* seg_lr, const float* seg_wd, int nseg, float max_norm, const void* workspace, float* norm_out);

/* ---- exponential moving average of the trainable bucket (still ABI 8: additive; optim.py, csrc/optim_ema.hip) --------------------------------------------------
 *   owl_ema_update      ema[i] = fma(d, ema[i], w * p[i]) on `stream`: exactly two f32 roundings per element (round-to-nearest intrinsics, whatever the
 *                       contraction flags).  d and w are formed by the caller: w = 1 - d, taken in double from the f32 d and rounded to f32.  n % 4 == 0;
 *                       no scratch, no atomics.  d = 0 (w = 1) gives ema == p and d = 1 (w = 0) leaves ema unchanged, bit for bit, for finite inputs.
 *   owl_adamw_step_ema  owl_adamw_step_grouped (same arguments, same clip prologue, same segment table, same bits in p / m / v / p_bf16) with the line
 *                       above applied to the just-updated parameter before it is stored: one more f32 stream in and one out, p is not read again.
 *                       Here a null seg_end means one segment over everything with the scalar `lr` / `weight_decay` (nseg is then ignored).           */
int owl_ema_update(void* stream, float* ema, const float* p, int64_t n, float d, float w);
int owl_adamw_step_ema(void* stream, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale, const int64_t* seg_end, const float* seg_lr, const float* seg_wd, int nseg, float max_norm, const void* workspace, float* norm_out, float* ema, float d, float w);

/* ---- frozen-prefix activation cache (still ABI 8: additive; prefix_cache.py, csrc/prefix_cache.hip) -------------------------------------------------------------
 * Under a freeze rule the residual stream that the first non-frozen consumer normalises depends on the pixels alone: it is kept per image (f32 blocks of
 * block_elems = Tp D elements) and the frozen layers below it are skipped for images already kept.
 *   owl_prefix_emit    for each of n freshly computed images j: s = (xs[j] + delta1[j]) + delta2[j] -- block j of the COMPACTED operands xs (f32) and
 *                      delta1 / delta2 (bf16, optional; delta2 only with delta1): the operands, the order and the plain f32 adds of owl_add_layernorm_fwd, so
 *                      its no-delta form on s gives the bits of its delta form on the operands -- written to dst_addr[j] and, where slot_addr[j] != 0, to
 *                      slot_addr[j] as well.  No destination may overlap xs (refused).
 *   owl_prefix_gather  for each of n kept images j: the block at src_addr[j] is copied to dst_addr[j] (one source may serve several destinations).
 * dst_addr / slot_addr / src_addr are HOST arrays of n DEVICE addresses, read by this call and passed to the kernels by value (no host-to-device copy,
 * no sync); 64 images per launch, longer lists take several launches.  Every address and block 16-byte aligned: block_elems % 8 == 0.  No atomics, no
 * scratch: pure streams.                                                                                                                            */
int owl_prefix_emit(void* stream, const float* xs, const void* delta1_bf16, const void* delta2_bf16, int64_t n, int64_t block_elems, const int64_t* dst_addr, const int64_t* slot_addr);
int owl_prefix_gather(void* stream, int64_t n, int64_t block_elems, const int64_t* src_addr, const int64_t* dst_addr);

/* ---- query bank from image exemplars (still ABI 8: additive; csrc/image_query.hip, models.OwlViT.embed_image_query / set_queries_from_exemplars) ----
 * OWL-ViT's image-conditioned query (HF5:1246-1288 `embed_image_query`), extended from HF's hard-wired whole image to a query box inside the example
 * image.  Initialisation-time entries: they run once, outside every step.
 *   owl_image_query_select   per exemplar n of N:  e f32 [N, P, Dt] (the class head's un-normalised dense0 output), boxes f32 [N, P, 4] corners,
 *       qbox f32 [N, 4] corners normalised to the processed image (NULL = [0, 0, 1, 1] for every exemplar: HF's literal rule).  HF's rule, quirks kept:
 *         1. iou_p = box_iou(qbox, boxes_p) in f32, one rounding per written operation (contraction off): both areas, lt = max, rb = min,
 *            wh = clamp(rb - lt, 0), inter, union = (area_q + area_p) - inter, inter / union;
 *         2. every iou_p == 0: v_p = iou_p - (hull_p - union_p) / hull_p (generalized_box_iou), else v_p = iou_p;
 *         3. thr = fl32(max_p v_p * 0.8f), selected = {p : v_p >= thr}; a negative maximum selects nothing (HF drops the image; here: EMPTY), after the
 *            fallback v_p <= 0, so only an exactly touching box (v_p == 0) is selected; a NaN v_p (zero-area box or hull) gives EMPTY, as torch.max would;
 *         4. mean_k = (sum over ALL p of e[p, k]) / P;   5. sim_p = sum_k mean_k e[p, k] for selected p;
 *         6. best = the selected p of smallest sim_p, the LOWEST p on a tie (torch.argmin).
 *       Steps 4 to 6 accumulate in float64 (f32 widened, f64 adds / FMAs, one fixed order -- as owl_grad_sumsq and the mAP IoU do): with f32 accumulation
 *       the worst-case error of a P-term column sum through a Dt-term dot is 1e-4 .. 5e-2 at P = 3600, Dt = 768, above the argmin margins of random
 *       inputs (2.5e-4), so no derived bound could decide the argmin; in f64 it is ~1e-13 and the kernels are bandwidth-bound either way.
 *       Outputs: best i32 [N] (-1 = empty); query f32 [N, Dt] = e[n, best] bit for bit (zeros when empty); info i32 [N, 2] = (flags: bit 0 fallback
 *       taken, bit 1 empty; number selected); optional diagnostics v_out f32 [N, P], mean_out f64 [N, Dt], sim_out f64 [N, P] (+inf where not selected).
 *       workspace: device scratch of owl_image_query_workspace_bytes(N, P, Dt) bytes (f64 column-sum partials, one per 64 rows); nothing is allocated.
 *       1 <= N <= 2^20, 1 <= P <= 8192, Dt % 4 == 0, Dt <= 1024; rows 16-byte aligned.  Two launches, no atomics, no host sync, bitwise reproducible.
 *   owl_query_bank_fill      query f32 [N, Dt]; a CSR assignment row_ptr i32 [nq + 1], members i32 (exemplar indices, ascending within a row), both on
 *       the DEVICE; bank f32 [nq, Dt].  Every row r with members: bank[r] = unit(sum over its members, ascending, of unit(query_m)), unit(x) = x / |x|,
 *       norms and sums in f64, ONE rounding to f32.  Rows without members are not touched.  One workgroup per row, no atomics.  nq <= 1152, Dt as above. */
int owl_image_query_workspace_bytes(int64_t N, int64_t P, int64_t Dt, int64_t* nbytes);
int owl_image_query_select(void* stream, const float* e, const float* boxes, const float* qbox, int64_t N, int64_t P, int64_t Dt, void* workspace, int64_t workspace_bytes, int* best, float* query, int* info, float* v_out, double* mean_out, double* sim_out);
int owl_query_bank_fill(void* stream, const float* query, const int* row_ptr, const int* members, float* bank, int64_t N, int64_t nq, int64_t Dt);

/* ---- open-vocabulary class head, forward (still ABI 8: additive; csrc/open_vocab.hip, models.OwlViT.detect / detect_text / forward_queries) ----------
 * HF's OwlViTClassPredictionHead over query banks that differ per image (text prompts, or an image exemplar's embedding).  Its adjoint is
 * owl_class_logits_bwd below (fine-tuning through this head: models.OwlViT.forward_queries); the bank head's kernels are untouched.  For image b, patch p, query q:
 *     e^_p     = e_p / (|e_p| + 1e-6)              e  f32 [B P, Dt]: the class head's dense0 output
 *     q^_{b,q} = Q_{b,q} / (|Q_{b,q}| + 1e-6)      queries f32 [nbanks, Q, Dt], nbanks = B (a bank per image) or 1 (one bank for the batch).  HF's epsilon
 *                                                  placement, not owl_query_normalize's; an all-zero row (HF's padded query) stays all-zero, never NaN
 *     shift_p  = w_shift . f_p + b_shift           feats bf16 [B P, D]: post_post_layernorm's output; w_shift / w_scale f32 [D]; b_shift / b_scale f32 [1]
 *     scale_p  = elu(w_scale . f_p + b_scale) + 1  on the DEVICE
 *     logits[b, p, q] = (e^_p . q^_{b,q} + shift_p) * scale_p, in this order; finfo(f32).min (-FLT_MAX) where mask[b, q] == 0
 *     scores[b, p, q] = 1 / (1 + exp(-logit)), exactly 0 where masked (scores may be NULL)
 *   mask u8 [nmasks, Q], nmasks = B or 1, nonzero = valid (HF's query_mask); NULL = every query valid.  logits / scores f32 [B, P, Q].
 *   rowstats f32 [B P, 2]: caller's scratch; a pre-pass writes (shift_p, scale_p) there once per row -- f32 FMAs over the widened bf16 features in one
 *   fixed order -- and every block of 32 queries reads those bits.  The cosine term runs on v_mfma_f32_32x32x2f32 with a 32-query table in LDS
 *   ([32][Dt + 4] f32), normalised while it is loaded; 32-row tiles never straddle two images.
 *   1 <= Q <= 4096, Dt % 64 == 0 (Dt <= 1024: the table must fit LDS), D % 8 == 0, 1 <= P <= 8192, 1 <= B P < 2^31; e, queries, feats, w_shift, w_scale
 *   16-byte aligned.  Two launches, no atomics, nothing allocated, no host sync; two runs give equal bits, and an image's block or a query's column
 *   carries the same bits wherever it stands in the batch or the bank.                                                                               */
int owl_class_logits_fwd(void* stream, const float* e, const float* queries, const void* feats_bf16, const float* w_shift, const float* b_shift, const float* w_scale, const float* b_scale, const unsigned char* mask, float* rowstats, float* logits, float* scores, int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t nmasks, int64_t Dt, int64_t D);

/* ---- open-vocabulary class head, backward (still ABI 8: additive; csrc/open_vocab_bwd.hip, models.OwlViT.forward_queries) ----------------------------
 * The adjoint of owl_class_logits_fwd on the forward's operands: e, queries, mask as there, rowstats f32 [B P, 2] = the (shift, scale) the forward left.
 * With g = dlogits f32 [B, P, Q] SELECTED to 0 where mask[b, q] == 0 (Inf / NaN there changes nothing), for row r of image b:
 *     T_r = sum_q g[r, q] q^_{b,q}     gs_r = sum_q g[r, q]     c_r = e^_r . T_r     (= sum_q g cos; the cosine term is never recovered as logit / scale)
 *     dshift = scale gs    dscale = c + shift gs    ds = dscale (scale > 1 ? 1 : scale)          ELU' read from the saved scale
 *     dfeats f32 [B P, D]  = dshift w_shift + ds w_scale: a plain store of the shift / scale term (may be NULL: not formed)
 *     de bf16 [B P, Dt]    = inv scale (T - e c / |e|), inv = 1 / (|e| + 1e-6); an all-zero row of e gives d(e^) / 1e-6, never NaN; finite where scale = 0
 *     dqueries f32 [nbanks, Q, Dt] = (dq^ - u (q^ . dq^)) / (|Q| + 1e-6), dq^_{b,q} = sum over image b's rows (a shared bank: every image's) of
 *                            g[r, q] inv_r scale_r e_r, u = Q / |Q| (0 for an all-zero row).  Plain store; a masked query's row is exactly 0.  May be NULL: the
 *                            work is skipped and de / dfeats keep their bits.
 *   T and dq^ run on v_mfma_f32_32x32x2f32 (f32 operands throughout); dq^ is summed per chunk of an image's rows into slabs of the workspace, which are
 *   added in index order.  32-row tiles never straddle two images; rows >= B P of every output are not written.  Four launches (two without dqueries), no
 *   atomics, nothing allocated, no host sync; every summation order is a function of (P, Q, Dt) alone: two runs give equal bits and an image's blocks are
 *   the same alone or anywhere in the batch.  workspace: owl_class_logits_bwd_workspace_bytes(..., want_dq = dqueries != NULL), 16-byte aligned, contents
 *   irrelevant.  Limits: the forward's (1 <= Q <= 4096, Dt % 64 == 0, Dt <= 1024, D % 8 == 0, 1 <= P <= 8192); w_shift, w_scale, dfeats 16-byte aligned. */
int owl_class_logits_bwd_workspace_bytes(int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t Dt, int want_dq, int64_t* bytes);
int owl_class_logits_bwd(void* stream, const float* dlogits, const float* e, const float* queries, const float* w_shift, const float* w_scale, const float* rowstats, const unsigned char* mask, void* workspace, int64_t workspace_bytes, void* de_bf16, float* dfeats, float* dqueries, int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t nmasks, int64_t Dt, int64_t D);

/* ---- open-vocabulary class head, backward with the gradients of the head's own tensors (still ABI 8: additive; csrc/open_vocab_bwd.hip) ---------------
 * owl_class_logits_bwd plus the gradients of logit_shift / logit_scale (models.OwlViT.set_logit_head(head, trainable=True)).  Every operand and output of
 * owl_class_logits_bwd means what it means there and carries the same bits; in addition
 *     feats bf16 [B P, D]: the features the forward read (16-byte aligned);  rowgrad f32 [B P, 2]: caller's scratch (8-byte aligned), (dshift_r, ds_r)
 *     of every row afterwards -- the row pass stores the two scalars it multiplies into dfeats; rows >= B P are not written
 *     dw_shift[c] = sum_r dshift_r feats[r, c]    db_shift = sum_r dshift_r    dw_scale[c] = sum_r ds_r feats[r, c]    db_scale = sum_r ds_r
 *     dw_shift / dw_scale f32 [D], db_shift / db_scale f32 [1]: plain stores, r over all B P rows.  dfeats and dqueries may be NULL as before: the four
 *     gradients keep their bits.
 *   Two more launches.  The first: one workgroup per (image, chunk of 256 rows, block of 128 columns), 16 row lanes x 16 column lanes, a thread reads 8
 *   bf16 features (16 bytes) per row and adds dshift f and ds f in FLOAT64 -- a bf16 times an f32 is exact there, so only the adds round -- and writes one
 *   f64 partial per workgroup into the workspace.  The second adds an image's partials in chunk order, then the images' sums in image order, and
 *   rounds ONCE to f32.  No atomics, nothing allocated, no host sync; the chunking depends on nothing (256 rows), so an image's partials carry the same
 *   bits wherever the image stands and two runs give equal bits.  Rows >= B P of feats and rowgrad are never read.
 *   workspace: owl_class_logits_bwd_head_workspace_bytes(..., want_dq = dqueries != NULL) = owl_class_logits_bwd's plus 8 B ceil(P / 256) (2 D + 2) bytes.
 *   Limits: owl_class_logits_bwd's, and D <= 2^20.                                                                                                      */
int owl_class_logits_bwd_head_workspace_bytes(int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t Dt, int64_t D, int want_dq, int64_t* bytes);
int owl_class_logits_bwd_head(void* stream, const float* dlogits, const float* e, const float* queries, const void* feats_bf16, const float* w_shift, const float* w_scale, const float* rowstats, const unsigned char* mask, void* workspace, int64_t workspace_bytes, float* rowgrad, void* de_bf16, float* dfeats, float* dqueries, float* dw_shift, float* dw_scale, float* db_shift, float* db_scale, int64_t B, int64_t P, int64_t Q, int64_t nbanks, int64_t nmasks, int64_t Dt, int64_t D);

/* ---- open-vocabulary criterion (still ABI 8: additive; csrc/open_vocab_loss.hip, losses.OpenVocabLoss / matcher.OpenVocabMatcher) -------------------
 * The DETR-family bipartite loss with sigmoid focal classification over the logits of owl_class_logits_fwd: transformers' DeformableDetrHungarianMatcher
 * and DeformableDetrImageLoss(losses = labels, boxes) on (logits, corners_to_center(boxes)), for per-image query lists.  Shared operands:
 *   logits f32 [B, P, Q] (-FLT_MAX under the mask); mask u8 [nmasks, Q], nmasks = B or 1, NULL = every query valid; boxes f32 [B, P, 4] corners;
 *   labels i64 [B, Nmax], tgt_boxes f32 [B, Nmax, 4] corners, counts i32 [B] (matcher.PackedTargets; counts[b] = 0 is legal); a label indexes the image's
 *   own query list, 0 <= label < Q.  Centre forms are taken inside the kernels: cx = (x0 + x1) / 2, w = x1 - x0; gradients come back on the corners.
 *   owl_focal_match_cost   costT f32 [B, Nmax, P] (owl_hungarian's layout; rows j >= counts[b] are not written), with p = sigmoid(logits[b, p, label_j]):
 *       w_bbox L1(centre forms) + w_class (alpha (1 - p)^2 (-log(p + 1e-8)) - (1 - alpha) p^2 (-log(1 - p + 1e-8))) + w_giou (-GIoU(corners)).
 *       A label outside [0, Q) or on a masked query never indexes the logits: class term 0 here, loss_ce NaN below.  Then owl_hungarian with bg = Q.
 *   owl_focal_loss_fwd     one f64 partial per workgroup of sum over (b, p, live q) of alpha_t softplus(z) sigmoid(z)^2, z = t ? -x : x,
 *       t = (target_classes[b, p] == q): HF's sigmoid_focal_loss term at gamma = 2, with 1 - p_t evaluated as sigmoid(z).  alpha < 0: no alpha weighting.
 *       Reads the logits once, 16 bytes per lane where Q % 4 == 0 (logits 16-byte aligned then).  Masked columns are selected out, never multiplied.
 *   owl_box_pair_loss      per image, over the matched pairs (pred_idx, tgt_idx i64 [B, Nmax] of owl_hungarian): sum L1 on centre forms, sum 1 - GIoU, and
 *       the unscaled gradients dl1, dgiou f32 [B, P, 4] wrt the corners, zero on unmatched rows (both NULL: not formed); torch's tie and sign(0) conventions.
 *   owl_open_vocab_loss_reduce   losses f32 [3] = (loss_ce, loss_bbox, loss_giou) = the three sums / num_boxes, partials added in one fixed order.
 *   owl_focal_loss_bwd     dlogits f32 [B, P, Q] = (g3[0] / num_boxes) d element / dx, recomputed from x and t; exactly +0.0 under the mask; reads the logits
 *       once and writes dlogits once.  g3 f32 [3] on the DEVICE = the upstream gradients of the three losses.
 *   owl_box_pair_loss_bwd  dboxes f32 [B, P, 4] = (g3[1] dl1 + g3[2] dgiou) / num_boxes.
 *   workspace: owl_focal_loss_workspace_bytes(B, P, Q), 8-byte aligned, written by owl_focal_loss_fwd and owl_box_pair_loss, read by the reduce.
 *   num_boxes: a positive HOST double.  Sums are f64 (thread, wave butterfly, workgroup partial); no atomics, nothing allocated, no host sync; every
 *   summation order is a function of (B, P, Q) alone: two runs give equal bits.  1 <= Q <= 4096, 1 <= P <= 8192, 1 <= Nmax <= P, B P < 2^31.             */
int owl_focal_match_cost(void* stream, const float* logits, const unsigned char* mask, const float* boxes, const int64_t* labels, const float* tgt_boxes, const int* counts, float* costT, int64_t B, int64_t P, int64_t Q, int64_t nmasks, int64_t Nmax, float alpha, float w_class, float w_bbox, float w_giou);
int owl_focal_loss_workspace_bytes(int64_t B, int64_t P, int64_t Q, int64_t* bytes);
int owl_focal_loss_fwd(void* stream, const float* logits, const unsigned char* mask, const int64_t* target_classes, void* workspace, int64_t workspace_bytes, int64_t B, int64_t P, int64_t Q, int64_t nmasks, float alpha);
int owl_box_pair_loss(void* stream, const float* boxes, const unsigned char* mask, const int64_t* labels, const float* tgt_boxes, const int64_t* pred_idx, const int64_t* tgt_idx, const int* counts, void* workspace, int64_t workspace_bytes, float* dl1, float* dgiou, int64_t B, int64_t P, int64_t Q, int64_t nmasks, int64_t Nmax);
int owl_open_vocab_loss_reduce(void* stream, const void* workspace, int64_t workspace_bytes, float* losses, int64_t B, int64_t P, int64_t Q, double num_boxes);
int owl_focal_loss_bwd(void* stream, const float* g3, const float* logits, const unsigned char* mask, const int64_t* target_classes, float* dlogits, int64_t B, int64_t P, int64_t Q, int64_t nmasks, float alpha, double num_boxes);
int owl_box_pair_loss_bwd(void* stream, const float* g3, const float* dl1, const float* dgiou, float* dboxes, int64_t B, int64_t P, double num_boxes);

/* ---- utilities ------------------------------------------------------------------------------------ */
int owl_cast_f32_bf16(void* stream, const float* in, void* out, int64_t n);
int owl_transpose_bf16(void* stream, const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t R, int64_t C);

#ifdef __cplusplus
}
#endif
#endif /* OWL_HIP_H */
