// The planner of the bf16 MFMA GEMM family: which kernels run a call of owl_gemm_nt_bf16, on which rows.  Host only, no HIP call.
#pragma once
#include "gemm_common.h"
#include "../../include/owl_hip.h"           // OWL_GEMM_KERNEL_*: the ids the planner speaks in
#ifdef OWL_TUNING
#include "../../include/owl_hip_tuning.h"
#endif

// Every routing rule of the family lives HERE, once: gemm.hip launches what gemm_plan returns, owl_gemm_nt_plan reports it, and
// tests/gemm_reference.py::dispatch_path is the independent Python restatement the tests hold it to.  Arguments are the VALIDATED ones of the call
// (gemm.hip, gemm_nt_check: split-K only on an epilogue with a slab, aux given where it is read, ...).
struct GemmPlan {
    int n;                                   // 1, or 2: rows [0, rows[0]) on kernel[0], the remaining rows[1] on kernel[1]
    int kernel[2];                           // OWL_GEMM_KERNEL_*
    int64_t rows[2];
};

// The epilogues each ping-pong kernel is instantiated for -- the `switch` of its launcher, which treats any other as an internal error.
constexpr bool pp2_takes(int epi) {          // gemm_pp2.hip (the transposing epilogue stays on the four-phase kernel of a tuning build)
    return epi == EPI_BIAS_BF16 || epi == EPI_QGELU_BF16 || epi == EPI_DQGELU_BF16 || epi == EPI_GELU_BF16 || epi == EPI_DGELU_BF16 || epi == EPI_F32 ||
           epi == EPI_ACC_F32 || epi == EPI_PATCH_F32 || epi == EPI_PATCHM_F32;
}
constexpr bool pph_takes(int epi) {          // gemm_pph.hip: the bf16 outputs
    return epi == EPI_BIAS_BF16 || epi == EPI_QGELU_BF16 || epi == EPI_DQGELU_BF16 || epi == EPI_GELU_BF16 || epi == EPI_DGELU_BF16;
}
#ifdef OWL_TUNING
constexpr bool pp4_takes(int epi) { return (pp2_takes(epi) && epi != EPI_PATCH_F32 && epi != EPI_PATCHM_F32) || epi == EPI_TRANS_BF16; }   // gemm_pp.hip
constexpr bool fr_takes(int epi) { return pp4_takes(epi) && epi != EPI_TRANS_BF16; }                                                       // gemm_fr.hip
constexpr bool w4_takes(int epi) { return epi == EPI_BIAS_BF16 || epi == EPI_QGELU_BF16; }                                                 // gemm_w4.hip
#endif
// split-K (EPI_SLAB_F32; EPI_ATOMIC_F32 of a tuning build) reaches the single-phase kernels only: no ping-pong kernel has those epilogues
static_assert(!pp2_takes(EPI_SLAB_F32) && !pp2_takes(EPI_ATOMIC_F32) && !pph_takes(EPI_SLAB_F32) && !pph_takes(EPI_ATOMIC_F32), "split-K is single-phase");

constexpr int64_t gemm_tiles256(int64_t M, int64_t N) { return ((M + 255) / 256) * ((N + 255) / 256); }

// "Big": 256-wide tiles only when they give the chip enough work items (batch-1 out-proj is 10 x 3 of them: the 128 x 128 kernel's 114 tiles finish sooner).
constexpr bool gemm_auto_big(int64_t M, int64_t N) { return M >= 512 && N >= 256 && gemm_tiles256(M, N) >= 48; }

// The single-phase kernel for `tile` (0 = by size; 256, and 8 / 9 of a tuning build, pin the 256 x 256 one; every other value the 128 x 128 one).
constexpr int gemm_single_phase(int64_t M, int64_t N, int tile) {
    return (tile ? (tile == 256 || tile == 8 || tile == 9) : gemm_auto_big(M, N)) ? OWL_GEMM_KERNEL_SP256 : OWL_GEMM_KERNEL_SP128;
}

// Tile quantisation: tm x tn tiles of 256 x 256 on 256 workgroups = full_rounds whole rounds + a remainder round that keeps only `rem` CUs busy
// (N = 768: 867 tiles = 3.39 -> 4 rounds).  When the remainder fits one round of HALF-height tiles the whole rounds go to the 256 x 256 ping-pong kernel
// and the remaining row tiles to the 128 x 256 variant (gemm_pph.hip): one round of ~0.56 tile times instead of a whole one.  Same K order and epilogue:
// bit-identical.  Returns the rows of the whole rounds (M_main), 0 = no such split.
constexpr int64_t gemm_whole_round_rows(int64_t M, int64_t N) {
    const int64_t tm = (M + 255) / 256, tn = (N + 255) / 256, items = tm * tn;
    const int64_t full_rounds = items / NUM_CUS;
    const int64_t tm_main = (full_rounds * NUM_CUS) / tn;
    const int64_t rem_tiles = (tm - tm_main) * tn;
    const bool fits = full_rounds >= 1 && tm_main >= 1 && rem_tiles > 0 && 2 * rem_tiles <= NUM_CUS && items - full_rounds * NUM_CUS > 0;
    return fits ? tm_main * 256 : 0;
}

// tile: 0 automatic | 6 automatic + half-height tiles for a small problem | 7 two-phase ping-pong on the whole problem | 128 / 256 the single-phase
// kernels (tuning builds: 8 / 9 the four-phase ping-pong kernel without / with the remainder split, 5 free-running, 4 four-wave).  `four_phase`: the
// owl_gemm_debug_nostore switch of a tuning build is set (its store skipping lives in the four-phase kernel); always false in the shipped library.
inline GemmPlan gemm_plan(int epi, int64_t M, int64_t N, int64_t K, int64_t a_rows, int tile, bool four_phase = false) {
    const auto whole = [&](int kernel) { return GemmPlan{1, {kernel, 0}, {M, 0}}; };
    const bool want_half = tile == 6;
    const int ft = want_half ? 0 : tile;
    const GemmPlan single = whole(gemm_single_phase(M, N, ft));
    if (K < 128) return single;                                  // every other kernel's pipeline needs two K-tiles
#ifdef OWL_TUNING
    if (ft == 4) return w4_takes(epi) ? whole(OWL_GEMM_KERNEL_W4) : single;
    if (ft == 5) return fr_takes(epi) ? whole(OWL_GEMM_KERNEL_FR) : single;
#endif
    if (ft == 7) return pp2_takes(epi) ? whole(OWL_GEMM_KERNEL_PP2) : single;
    // bf16-output (and the f32 head) epilogues on big problems run a ping-pong schedule: 13-26 % faster than the single-phase kernel, bit-identical.  The
    // two-phase one (gemm_pp2.hip) where it has the epilogue: +3..9 % over the four-phase one on the model's shapes.
    int pp = pp2_takes(epi) ? OWL_GEMM_KERNEL_PP2 : -1;
    bool split = N <= 1024;                                      // (see below)
#ifdef OWL_TUNING                                                // tile 8 / 9, the store-skipping switch and the transposing epilogue: the four-phase kernel
    if (ft == 8 || ft == 9 || four_phase || pp < 0) pp = pp4_takes(epi) ? OWL_GEMM_KERNEL_PP4 : -1;
    if (ft == 8 || ft == 9) split = ft == 9;                     // tile 9 forces the remainder split wherever it fits, tile 8 never splits
    if (!(ft == 0 ? gemm_auto_big(M, N) : ft == 8 || ft == 9)) return single;
#else
    if (!(ft == 0 && gemm_auto_big(M, N))) return single;
#endif
    // tile = 6 -- small problems (the reference's own batch size of 1: QKV = 90 tiles, fc1 = 120 on 256 CUs): no more 256 x 256 tiles than HALF the CUs ->
    // every tile goes out as two half-height tiles (gemm_pph.hip), one partial round of ~0.85 tile times on twice the CUs.  Same K order and epilogue:
    // bit-identical.  Asked for by the CALLER, who knows what else is in flight: with two sub-batch streams the other stream's tiles already fill the idle
    // CUs and the half-height split loses (forward batch 8: -2.7 %; alone: +3.3 % / +4.5 % on the batch-1 train step / forward, profiles/r05_small_batch.md).
    if (want_half && a_rows >= M && 2 * gemm_tiles256(M, N) <= NUM_CUS && pph_takes(epi)) return whole(OWL_GEMM_KERNEL_PPH);
    if (pp < 0) return single;
    // The remainder round on half-height tiles (gemm_whole_round_rows).  Measured (tools/gemm_remainder_bench.py, same-process A/B at M = 73 984): +3.6 % fc2
    // (K = 3072), +2.5 % dX (K = 2304), +4.2 % box-head dense (GELU epilogue), +0.8 % out-proj (K = 768); nothing for wide outputs (QKV N = 2304: -0.1 %,
    // fc1: does not fit one round), where the half-height tiles -- latency-bound, ~0.85 of a full tile's time, not 0.56 -- only just pay for the second
    // launch.  Hence the automatic rule: narrow outputs only (N <= 1024).  The f32 outputs (EPI_F32, EPI_ACC_F32) have no half-height kernel and stay whole.
    const int64_t M_main = (split && pph_takes(epi) && a_rows >= M) ? gemm_whole_round_rows(M, N) : 0;
    if (M_main) return GemmPlan{2, {pp, OWL_GEMM_KERNEL_PPH}, {M_main, M - M_main}};
    return whole(pp);
}
