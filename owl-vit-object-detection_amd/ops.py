"""Thin Python wrappers over the C ABI (include/owl_hip.h): shape/dtype validation, stream, call.

PyTorch is plumbing here (device memory + streams); every op below runs a hand-written HIP kernel
from libowlhip.so and raises if the library is missing -- there is no eager fallback.
"""
import torch

from . import _lib

EPI_BIAS_BF16, EPI_QGELU_BF16, EPI_GELU_BF16, EPI_RESID_F32, EPI_F32, EPI_ATOMIC_F32 = 0, 1, 2, 3, 4, 5
EPI_TRANS_BF16, EPI_PATCH_F32, EPI_DQGELU_BF16, EPI_DGELU_BF16, EPI_ACC_F32, EPI_SLAB_F32 = 6, 7, 8, 9, 10, 11

ROW_PAD = 128
CHIP_CUS = 256     # MI355X (gfx950), the only target: the kernels' persistent grids and the small-problem rule below count on it (csrc/gemm_common.h NUM_CUS);
                   # models.OwlViT warns when the device reports another count (a partitioned GPU)
ATTN_VARIANT = 0   # default `variant` of attention_fwd_vrow(): 0 = the library's choice; 1 plain tiling, 2 class token peeled (tests / tools)
GEMM_TILE = 0      # default `tile` argument of gemm(): 0 = automatic kernel choice; tests / tools pin one kernel (128 | 256 | 7; tuning builds: 8 | 9 | 5 | 4)


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def pad_rows(n: int) -> int:
    return (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD


def zeros_rows(rows: int, width: int, dtype, device) -> torch.Tensor:
    """[pad_rows(rows), width] zero buffer (pad rows stay zero / finite by construction)."""
    return torch.zeros(pad_rows(rows), width, dtype=dtype, device=device)


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def gemm(epi, A, W, out, bias=None, resid=None, aux=None, M=None, N=None, K=None, lda=None, ldw=None, ldo=None,
         ld_aux=0, a_rows=None, w_rows=None, alpha=1.0, splits=1, Tp=0, tile=None, concurrency=None):
    """out = epilogue(A[M,K] @ W[N,K]^T).  A/W bf16; see include/owl_hip.h for epilogues.
    concurrency: how many launches like this one the caller has in flight at once (sub-batch streams).  If their 256 x 256 tiles together fill at most half
    the chip's CHIP_CUS compute units, the automatic kernel choice becomes tile 6 (half-height tiles; include/owl_hip.h): the library cannot know what else is running."""
    _chk(A, torch.bfloat16, "A"); _chk(W, torch.bfloat16, "W"); _chk(bias, torch.float32, "bias")
    K = K if K is not None else A.shape[-1]
    N = N if N is not None else W.shape[0]
    M = M if M is not None else A.shape[0]
    lda = lda if lda is not None else A.shape[-1]
    ldw = ldw if ldw is not None else W.shape[-1]
    ldo = ldo if ldo is not None else (out.shape[-1] if epi != EPI_TRANS_BF16 else 0)
    a_rows = a_rows if a_rows is not None else A.shape[0]
    w_rows = w_rows if w_rows is not None else W.shape[0]
    if aux is not None and ld_aux == 0:
        ld_aux = aux.shape[-1]
    tile = int(GEMM_TILE if tile is None else tile)
    if tile == 0 and concurrency is not None and 2 * int(concurrency) * ((M + 255) // 256) * ((N + 255) // 256) <= CHIP_CUS:
        tile = 6
    _lib.call("owl_gemm_nt_bf16", stream(), epi, A, lda, a_rows, W, ldw, w_rows, bias, out, ldo, resid, aux, ld_aux,
              M, N, K, float(alpha), int(splits), int(Tp), tile)
    return out


def patch_embed(image_bf16, w_pe, pos, x_out, B, S, ps, D, Tp, scratch=None, tile=0):
    _chk(image_bf16, torch.bfloat16, "image"); _chk(w_pe, torch.bfloat16, "w_pe"); _chk(pos, torch.float32, "pos")
    _chk(x_out, torch.float32, "x_out")
    _lib.call("owl_patch_embed_bf16", stream(), image_bf16, w_pe, pos, x_out, scratch, B, S, ps, D, Tp, int(tile))


def patch_embed_hw(image_bf16, w_pe, pos, x_out, B, H, W, ps, D, Tp, scratch=None, tile=0):
    """patch_embed on an image [B, 3, H, W]: patch y * (W / ps) + x goes to row b * Tp + 1 + p (the same kernels; H == W is patch_embed, bit for bit)."""
    _chk(image_bf16, torch.bfloat16, "image"); _chk(w_pe, torch.bfloat16, "w_pe"); _chk(pos, torch.float32, "pos")
    _chk(x_out, torch.float32, "x_out")
    _lib.call("owl_patch_embed_bf16_hw", stream(), image_bf16, w_pe, pos, x_out, scratch, B, H, W, ps, D, Tp, int(tile))


def cls_rows(x, cls, pos, B, Tp, D):
    _lib.call("owl_cls_rows", stream(), x, cls, pos, B, Tp, D)


def layernorm(x, gamma, beta, out, rows, D, stats=None, eps=1e-5, delta=None, x_out=None, delta2=None, store_x=True):
    """out = LN(x) -- or, with `delta` (bf16; optionally a second one), s = x + delta (+ delta2), out = LN(s) and
    x_out = s in one pass; `store_x=False` skips the write of s (the caller re-forms it later from the same operands)."""
    _chk(x, torch.float32, "x"); _chk(gamma, torch.float32, "gamma"); _chk(beta, torch.float32, "beta")
    ob = 1 if out.dtype == torch.bfloat16 else 0
    if delta is None:
        _lib.call("owl_layernorm_fwd", stream(), x, gamma, beta, out, ob, stats, rows, D, float(eps))
    else:
        _chk(delta, torch.bfloat16, "delta"); _chk(delta2, torch.bfloat16, "delta2")
        xo = (x_out if x_out is not None else x) if store_x else None
        _lib.call("owl_add_layernorm_fwd", stream(), x, delta, xo, gamma, beta, out, ob, stats, rows, D, float(eps), delta2)
    return out


def _tuning_only(what):
    if not _lib.is_tuning_build():
        raise RuntimeError(f"{what} exists only in an OWL_TUNING build of libowlhip.so (OWL_TUNING=1 bash csrc/build.sh); the loaded library is the shipped build")


def attention_fwd(q, k, ld_qk, vt, vt_img_stride, out, ld_out, lse, B, H, T, Tp, scale):
    """Tuning builds only: the round-1 form with V^T per head (include/owl_hip_tuning.h)."""
    _tuning_only("the V^T attention forward")
    _lib.call("owl_attention_fwd_bf16", stream(), q, k, ld_qk, vt, vt_img_stride, out, ld_out, lse, B, H, T, Tp,
              float(scale))
    return out


_attn_redo = {}


def attention_redo_ws(B, H, T, device):
    """Tuning builds only: scratch of the one-wave-per-SIMD attention forward (one int per query block; contents irrelevant): one buffer per (device, stream)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    n = B * H * ((T - 1 + 255) // 256 + 1)
    buf = _attn_redo.get(key)
    if buf is None or buf.numel() < n:
        buf = _attn_redo[key] = torch.zeros(max(n, 4096) + 8192, dtype=torch.int32, device=device)
    return buf


ATTN_SLOW_TILES = None   # optional int32[1] device tensor: every attention forward adds its count of slow-path tiles (bench.py --weights trained_like, tests)


def attention_fwd_vrow(q, k, v, ld_qkv, out, ld_out, lse, B, H, T, Tp, scale, variant=None, slow_tiles=None):
    """Fused attention forward; q / k / v are column slices of the row-major qkv rows (no V^T copy).  variant 0-2: include/owl_hip.h; 3-5: tuning builds."""
    variant = int(ATTN_VARIANT if variant is None else variant)
    if variant >= 3:
        _tuning_only(f"attention forward variant {variant}")
        _lib.call("owl_attention_fwd_w64_bf16", stream(), q, k, v, ld_qkv, out, ld_out, lse, B, H, T, Tp, float(scale), variant, attention_redo_ws(B, H, T, out.device))
        return out
    if slow_tiles is None:
        slow_tiles = ATTN_SLOW_TILES
    _lib.call("owl_attention_fwd_vrow_bf16", stream(), q, k, v, ld_qkv, out, ld_out, lse, B, H, T, Tp, float(scale), variant, slow_tiles)
    return out


def merge_ln(x, g1, b1, g2, b2, cls_ln, feats, stats1, stats2, B, P, Tp, D, eps=1e-5, delta=None, x_out=None):
    _lib.call("owl_merge_ln_fwd", stream(), x, delta, (x_out if x_out is not None else x) if delta is not None else None,
              g1, b1, g2, b2, cls_ln, feats, stats1, stats2, B, P, Tp, D, float(eps))


def query_normalize(queries, qhat32, qnorm, nq, Dt):
    _chk(queries, torch.float32, "queries")
    _lib.call("owl_query_normalize", stream(), queries, qhat32, qnorm, nq, Dt)


def class_sims(e, qhat32, sims, argmax, inv_norm, rows, Dt, C):
    _chk(e, torch.float32, "e")
    _lib.call("owl_class_sims_fwd", stream(), e, qhat32, sims, argmax, inv_norm, rows, Dt, C)


WIDE_MAX_CLASSES = 384     # ceiling of the wide class head (csrc/common.h OWL_WIDE_MAX_CLASSES)


def wide_blocks(C: int) -> int:
    """Query blocks (10 classes = 30 prompts in a 32-row MFMA tile) of the wide class head's [nblk][32][Dt] layout."""
    return (int(C) + 9) // 10


def wide_qp(C: int) -> int:
    """Columns of the wide class head's routed upstream G [rows, Qp]: 32 per query block, rounded up to the TN weight-gradient kernel's 256."""
    return (32 * wide_blocks(C) + 255) // 256 * 256


def query_normalize_wide(queries, qhat_wide, qnorm, nq, Dt):
    _chk(queries, torch.float32, "queries"); _chk(qhat_wide, torch.float32, "qhat_wide")
    if qhat_wide.numel() < 32 * wide_blocks(nq // 3) * Dt:
        raise ValueError("query_normalize_wide: qhat_wide must hold [ceil(C / 10) * 32, Dt] floats")
    _lib.call("owl_query_normalize_wide", stream(), queries, qhat_wide, qnorm, nq, Dt)


def class_sims_wide(e, qhat_wide, sims, argmax, inv_norm, rows, Dt, C):
    _chk(e, torch.float32, "e"); _chk(qhat_wide, torch.float32, "qhat_wide")
    if qhat_wide.numel() < 32 * wide_blocks(C) * Dt:
        raise ValueError("class_sims_wide: qhat_wide must hold [ceil(C / 10) * 32, Dt] floats")
    _lib.call("owl_class_sims_wide_fwd", stream(), e, qhat_wide, sims, argmax, inv_norm, rows, Dt, C)


CLASS_LOGITS_MAX_QUERIES = 4096     # ceiling of class_logits (csrc/open_vocab.hip OV_MAX_QUERIES)


def class_logits(e, queries, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask=None, rowstats=None, logits=None, scores=False):
    """HF's OwlViTClassPredictionHead over per-image query banks (include/owl_hip.h owl_class_logits_fwd; its adjoint is class_logits_bwd):
    logits[b, p, q] = (e^_p . q^_{b,q} + shift_p) * scale_p with HF's q / (|q| + 1e-6), finfo(f32).min where mask == 0.
    e f32 [>= B P, Dt]; queries f32 [B, Q, Dt] or [Q, Dt] (one bank for the batch, read where it lies); feats bf16 [>= B P, D]; w_shift / w_scale f32 [D];
    b_shift / b_scale f32 device tensors of one element; mask uint8 [B, Q] or [Q] (nonzero = valid) or None.  rowstats (f32 [>= B P, 2] scratch: (shift,
    scale) per row afterwards) and logits (f32 [B, P, Q]) are allocated when not given; scores: False, True (allocate) or an f32 [B, P, Q] tensor.
    -> (logits, scores or None, rowstats).  No host sync."""
    _chk(e, torch.float32, "e"); _chk(queries, torch.float32, "queries"); _chk(feats, torch.bfloat16, "feats")
    _chk(w_shift, torch.float32, "w_shift"); _chk(b_shift, torch.float32, "b_shift"); _chk(w_scale, torch.float32, "w_scale"); _chk(b_scale, torch.float32, "b_scale")
    _chk(mask, torch.uint8, "mask"); _chk(rowstats, torch.float32, "rowstats"); _chk(logits, torch.float32, "logits")
    B, P = int(B), int(P)
    if queries.dim() not in (2, 3) or (queries.dim() == 3 and queries.shape[0] != B):
        raise ValueError(f"class_logits: queries must be [{B}, Q, Dt] or [Q, Dt], got {tuple(queries.shape)}")
    Q, Dt = int(queries.shape[-2]), int(queries.shape[-1])
    D = int(w_shift.numel())
    if e.dim() != 2 or e.shape[1] != Dt or e.shape[0] < B * P:
        raise ValueError(f"class_logits: e must be [>= {B * P}, {Dt}], got {tuple(e.shape)}")
    if feats.dim() != 2 or feats.shape[1] != D or feats.shape[0] < B * P or w_scale.numel() != D or b_shift.numel() != 1 or b_scale.numel() != 1:
        raise ValueError(f"class_logits: feats must be [>= {B * P}, D], w_shift / w_scale [D], b_shift / b_scale one element each (D = {D}, feats {tuple(feats.shape)})")
    if not 1 <= Q <= CLASS_LOGITS_MAX_QUERIES:
        raise ValueError(f"class_logits: 1 <= Q <= {CLASS_LOGITS_MAX_QUERIES} queries per image, got {Q}")
    if mask is not None and tuple(mask.shape) not in ((B, Q), (Q,)):
        raise ValueError(f"class_logits: mask must be [{B}, {Q}] or [{Q}], got {tuple(mask.shape)}")
    dev = e.device
    if rowstats is None:
        rowstats = torch.empty(B * P, 2, dtype=torch.float32, device=dev)
    elif rowstats.numel() < 2 * B * P:
        raise ValueError(f"class_logits: rowstats must hold [{B * P}, 2] floats")
    if logits is None:
        logits = torch.empty(B, P, Q, dtype=torch.float32, device=dev)
    elif tuple(logits.shape) != (B, P, Q):
        raise ValueError(f"class_logits: logits must be [{B}, {P}, {Q}], got {tuple(logits.shape)}")
    if scores is True:
        scores = torch.empty(B, P, Q, dtype=torch.float32, device=dev)
    elif scores is False:
        scores = None
    else:
        _chk(scores, torch.float32, "scores")
        if tuple(scores.shape) != (B, P, Q):
            raise ValueError(f"class_logits: scores must be [{B}, {P}, {Q}], got {tuple(scores.shape)}")
    _lib.call("owl_class_logits_fwd", stream(), e, queries, feats, w_shift, b_shift, w_scale, b_scale, mask, rowstats, logits, scores,
              B, P, Q, B if queries.dim() == 3 else 1, (B if mask.dim() == 2 else 1) if mask is not None else 1, Dt, D)
    return logits, scores, rowstats


def class_logits_bwd_workspace_bytes(B, P, Q, nbanks, Dt, want_dq=True):
    """Bytes of class_logits_bwd's workspace (include/owl_hip.h owl_class_logits_bwd_workspace_bytes): a host computation, no device is touched."""
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_class_logits_bwd_workspace_bytes", int(B), int(P), int(Q), int(nbanks), int(Dt), 1 if want_dq else 0, nbytes)
    return int(nbytes.item())


def class_logits_bwd_head_workspace_bytes(B, P, Q, nbanks, Dt, D, want_dq=True):
    """Bytes of class_logits_bwd's workspace where the head's own gradients are formed (dhead; include/owl_hip.h owl_class_logits_bwd_head_workspace_bytes)."""
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_class_logits_bwd_head_workspace_bytes", int(B), int(P), int(Q), int(nbanks), int(Dt), int(D), 1 if want_dq else 0, nbytes)
    return int(nbytes.item())


def class_logits_bwd(dlogits, e, queries, w_shift, w_scale, rowstats, B, P, mask=None, de=None, dfeats=True, dqueries=True, workspace=None, feats=None,
                     dhead=False, rowgrad=None):
    """The adjoint of class_logits (include/owl_hip.h owl_class_logits_bwd) on the forward's operands; rowstats is what that forward left.
    dlogits f32 [B, P, Q] (masked entries are selected to 0: anything may stand there); e f32 [>= B P, Dt]; queries f32 [B, Q, Dt] or [Q, Dt];
    w_shift / w_scale f32 [D]; rowstats f32 [>= B P, 2]; mask uint8 [B, Q] or [Q] or None.
    de: bf16 [>= B P, Dt], allocated when None.  dfeats / dqueries: True (allocate: f32 [B P, D] / f32 of queries' shape), False (not formed: the work
    is skipped) or the tensor to store into (dfeats f32 [>= B P, D]).  workspace: a uint8 device tensor of at least
    class_logits_bwd_workspace_bytes(...) bytes, allocated when None.  -> (de, dfeats or None, dqueries or None).  No host sync.

    dhead: False (today's entry, unchanged), True (allocate) or an f32 [2 D + 2] tensor laid out w_shift | w_scale | b_shift | b_scale: the gradients of
    the head's own four tensors (include/owl_hip.h owl_class_logits_bwd_head).  It needs feats, the bf16 [>= B P, D] features the forward read;
    rowgrad is the f32 [>= B P, 2] scratch that receives (dshift, ds) per row (allocated when None) and the workspace is
    class_logits_bwd_head_workspace_bytes(...) bytes.  -> (de, dfeats or None, dqueries or None, dhead) then."""
    _chk(dlogits, torch.float32, "dlogits"); _chk(e, torch.float32, "e"); _chk(queries, torch.float32, "queries")
    _chk(w_shift, torch.float32, "w_shift"); _chk(w_scale, torch.float32, "w_scale"); _chk(rowstats, torch.float32, "rowstats"); _chk(mask, torch.uint8, "mask")
    B, P = int(B), int(P)
    if queries.dim() not in (2, 3) or (queries.dim() == 3 and queries.shape[0] != B):
        raise ValueError(f"class_logits_bwd: queries must be [{B}, Q, Dt] or [Q, Dt], got {tuple(queries.shape)}")
    Q, Dt = int(queries.shape[-2]), int(queries.shape[-1])
    D = int(w_shift.numel())
    if tuple(dlogits.shape) != (B, P, Q):
        raise ValueError(f"class_logits_bwd: dlogits must be [{B}, {P}, {Q}], got {tuple(dlogits.shape)}")
    if e.dim() != 2 or e.shape[1] != Dt or e.shape[0] < B * P:
        raise ValueError(f"class_logits_bwd: e must be [>= {B * P}, {Dt}], got {tuple(e.shape)}")
    if w_scale.numel() != D:
        raise ValueError(f"class_logits_bwd: w_shift / w_scale must be [D] alike, got {w_shift.numel()} and {w_scale.numel()} elements")
    if not 1 <= Q <= CLASS_LOGITS_MAX_QUERIES:
        raise ValueError(f"class_logits_bwd: 1 <= Q <= {CLASS_LOGITS_MAX_QUERIES} queries per image, got {Q}")
    if rowstats.numel() < 2 * B * P:
        raise ValueError(f"class_logits_bwd: rowstats must hold [{B * P}, 2] floats")
    if mask is not None and tuple(mask.shape) not in ((B, Q), (Q,)):
        raise ValueError(f"class_logits_bwd: mask must be [{B}, {Q}] or [{Q}], got {tuple(mask.shape)}")
    dev = e.device
    if de is None:
        de = torch.empty(B * P, Dt, dtype=torch.bfloat16, device=dev)
    else:
        _chk(de, torch.bfloat16, "de")
        if de.dim() != 2 or de.shape[1] != Dt or de.shape[0] < B * P:
            raise ValueError(f"class_logits_bwd: de must be bf16 [>= {B * P}, {Dt}], got {tuple(de.shape)}")
    if dfeats is True:
        dfeats = torch.empty(B * P, D, dtype=torch.float32, device=dev)
    elif dfeats is False:
        dfeats = None
    else:
        _chk(dfeats, torch.float32, "dfeats")
        if dfeats.dim() != 2 or dfeats.shape[1] != D or dfeats.shape[0] < B * P:
            raise ValueError(f"class_logits_bwd: dfeats must be f32 [>= {B * P}, {D}], got {tuple(dfeats.shape)}")
    if dqueries is True:
        dqueries = torch.empty_like(queries)
    elif dqueries is False:
        dqueries = None
    else:
        _chk(dqueries, torch.float32, "dqueries")
        if tuple(dqueries.shape) != tuple(queries.shape):
            raise ValueError(f"class_logits_bwd: dqueries must be f32 {tuple(queries.shape)}, got {tuple(dqueries.shape)}")
    nbanks = B if queries.dim() == 3 else 1
    if dhead is False:
        if rowgrad is not None:
            raise ValueError("class_logits_bwd: rowgrad is the scratch of dhead (dhead=False forms no head gradients)")
        need, query = class_logits_bwd_workspace_bytes(B, P, Q, nbanks, Dt, dqueries is not None), "class_logits_bwd_workspace_bytes"
    else:
        if feats is None:
            raise ValueError("class_logits_bwd: dhead needs feats, the bf16 [>= B P, D] features the forward read")
        _chk(feats, torch.bfloat16, "feats")
        if feats.dim() != 2 or feats.shape[1] != D or feats.shape[0] < B * P:
            raise ValueError(f"class_logits_bwd: feats must be bf16 [>= {B * P}, {D}], got {tuple(feats.shape)}")
        if dhead is True:
            dhead = torch.empty(2 * D + 2, dtype=torch.float32, device=dev)
        else:
            _chk(dhead, torch.float32, "dhead")
            if tuple(dhead.shape) != (2 * D + 2,):
                raise ValueError(f"class_logits_bwd: dhead must be f32 [{2 * D + 2}] (w_shift | w_scale | b_shift | b_scale), got {tuple(dhead.shape)}")
        if rowgrad is None:
            rowgrad = torch.empty(B * P, 2, dtype=torch.float32, device=dev)
        else:
            _chk(rowgrad, torch.float32, "rowgrad")
            if rowgrad.numel() < 2 * B * P:
                raise ValueError(f"class_logits_bwd: rowgrad must hold [{B * P}, 2] floats")
        need, query = class_logits_bwd_head_workspace_bytes(B, P, Q, nbanks, Dt, D, dqueries is not None), "class_logits_bwd_head_workspace_bytes"
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        _chk(workspace, torch.uint8, "workspace")
        if workspace.numel() < need:
            raise ValueError(f"class_logits_bwd: workspace must hold {need} bytes ({query}), got {workspace.numel()}")
    nmasks = (B if mask.dim() == 2 else 1) if mask is not None else 1
    if dhead is not False:
        _lib.call("owl_class_logits_bwd_head", stream(), dlogits, e, queries, feats, w_shift, w_scale, rowstats, mask, workspace, need, rowgrad, de, dfeats,
                  dqueries, dhead[:D], dhead[D:2 * D], dhead[2 * D:2 * D + 1], dhead[2 * D + 1:], B, P, Q, nbanks, nmasks, Dt, D)
        return de, dfeats, dqueries, dhead
    _lib.call("owl_class_logits_bwd", stream(), dlogits, e, queries, w_shift, w_scale, rowstats, mask, workspace, need, de, dfeats, dqueries,
              B, P, Q, nbanks, (B if mask.dim() == 2 else 1) if mask is not None else 1, Dt, D)
    return de, dfeats, dqueries


def box_final(h, w2, b2, box_bias, boxes, sig, rows, P, D):
    _chk(h, torch.bfloat16, "h"); _chk(w2, torch.float32, "w2")
    _lib.call("owl_box_final_fwd", stream(), h, w2, b2, box_bias, boxes, sig, rows, P, D)


def cast_bf16(src, dst=None):
    _chk(src, torch.float32, "src")
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    _lib.call("owl_cast_f32_bf16", stream(), src, dst, src.numel())
    return dst


def transpose_bf16(src, dst, R, C, ld_in=None, ld_out=None):
    _lib.call("owl_transpose_bf16", stream(), src, ld_in if ld_in is not None else src.shape[-1], dst,
              ld_out if ld_out is not None else dst.shape[-1], R, C)
    return dst


# ---- frozen-prefix activation cache (csrc/prefix_cache.hip) -------------------------------------------------
def _addr_table(addrs):
    """Host int64 array of device addresses (the library reads it during the call and hands it to the kernel by value: no device copy)."""
    return torch.tensor([int(a) for a in addrs], dtype=torch.int64)


def prefix_emit(xs, delta1, delta2, n, block_elems, dst_addr, slot_addr):
    """For each of the n images of the compacted batch: s = (xs[j] + delta1[j]) + delta2[j] (deltas bf16, optional) -> the f32 block at device address
    dst_addr[j] and, where slot_addr[j] != 0, at slot_addr[j].  dst_addr / slot_addr: sequences of n ints."""
    _chk(xs, torch.float32, "xs"); _chk(delta1, torch.bfloat16, "delta1"); _chk(delta2, torch.bfloat16, "delta2")
    n, block_elems = int(n), int(block_elems)
    if len(dst_addr) != n or len(slot_addr) != n:
        raise ValueError(f"prefix_emit: dst_addr / slot_addr must have n = {n} entries")
    for t, name in ((xs, "xs"), (delta1, "delta1"), (delta2, "delta2")):
        if t is not None and t.numel() < n * block_elems:
            raise ValueError(f"prefix_emit: {name} must hold n blocks of {block_elems} elements")
    _lib.call("owl_prefix_emit", stream(), xs, delta1, delta2, n, block_elems, _addr_table(dst_addr), _addr_table(slot_addr))


def prefix_gather(n, block_elems, src_addr, dst_addr):
    """For each of n images: the f32 block at device address src_addr[j] -> the block at dst_addr[j].  Sequences of n ints."""
    n = int(n)
    if len(src_addr) != n or len(dst_addr) != n:
        raise ValueError(f"prefix_gather: src_addr / dst_addr must have n = {n} entries")
    _lib.call("owl_prefix_gather", stream(), n, int(block_elems), _addr_table(src_addr), _addr_table(dst_addr))


# ---- backward-side wrappers ---------------------------------------------------------------------------
_partials = {}


def rowreduce_workspace(groups, rows_per_group, C, device):
    """f32 partial-sum scratch for the deterministic row reductions (owl_rowreduce_workspace_bytes)."""
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_rowreduce_workspace_bytes", int(groups), int(rows_per_group), int(C), nbytes)
    return torch.empty(int(nbytes.item()) // 4, dtype=torch.float32, device=device)


def part_floats(rows, C) -> int:
    """f32 elements of the partial-sum scratch a deterministic column reduction over `rows` rows of `C` columns takes (what _part allocates)."""
    return ((int(rows) + 63) // 64 + 1) * 6 * max(int(C), 4)


def _part(partials, rows, C, device):
    """The caller's scratch, or (stand-alone use: tests, tools) a cached per-device buffer grown on demand."""
    if partials is not None:
        return partials
    need = part_floats(rows, C)
    buf = _partials.get(device)
    if buf is None or buf.numel() < need:
        buf = torch.empty(need, dtype=torch.float32, device=device)
        _partials[device] = buf
    return buf


def layernorm_bwd(dy, x, stats, gamma, dres, dx, dgamma, dbeta, rows, D, dx_bf16=None, partials=None, dx_colsum=None):
    """dx (f32) = LN backward (+ dres); optionally also its bf16 copy `dx_bf16` (the operand of the next dX GEMM) and `dx_colsum` +=
    the column sums of dx (the bias gradient of the linear layer in front of this residual position)."""
    _chk(dx_bf16, torch.bfloat16, "dx_bf16"); _chk(dx_colsum, torch.float32, "dx_colsum")
    part = _part(partials, rows, D, x.device) if dgamma is not None else None
    _lib.call("owl_layernorm_bwd", stream(), dy, 1 if dy.dtype == torch.bfloat16 else 0, x, stats, gamma, dres, dx,
              dgamma, dbeta, rows, D, dx_bf16, part, part.numel() if part is not None else 0, dx_colsum)


def merge_ln_bwd(dfeats, x, cls_ln, st1, st2, g1, b1, g2, dx, dcls_ws, dg1, db1, dg2, db2, B, P, Tp, D, partials=None, dx_bf16=None, dx_colsum=None):
    """dx_colsum (optional): += column sums of dx over all tokens (the bias gradient of the last layer's fc2) in the same pass."""
    part = partials if partials is not None else _part(None, B * ((P + 63) // 64) * 64, D, x.device)
    _chk(dx_bf16, torch.bfloat16, "dx_bf16"); _chk(dx_colsum, torch.float32, "dx_colsum")
    _lib.call("owl_merge_ln_bwd", stream(), dfeats, x, cls_ln, st1, st2, g1, b1, g2, dx, dcls_ws, dg1, db1, dg2, db2, B, P, Tp, D,
              part, part.numel(), dx_bf16, dx_colsum)


def class_sims_bwd(dsims, sims, argmax, inv_norm, e, qhat32, de, g32, e_bf16, rows, Dt, C):
    _lib.call("owl_class_sims_bwd", stream(), dsims, sims, argmax, inv_norm, e, qhat32, de, g32, e_bf16, rows, Dt, C)


def class_sims_wide_bwd(dsims, sims, argmax, inv_norm, e, qhat_wide, de, g, e_bf16, rows, Dt, C):
    """g: bf16 [>= rows, wide_qp(C)] (every element of the first `rows` rows is written)."""
    _chk(g, torch.bfloat16, "g"); _chk(de, torch.bfloat16, "de"); _chk(e_bf16, torch.bfloat16, "e_bf16")
    Qp = wide_qp(C)
    if g.shape[-1] != Qp or g.numel() < rows * Qp or de.numel() < rows * Dt or e_bf16.numel() < rows * Dt:
        raise ValueError(f"class_sims_wide_bwd: g must be [rows, {Qp}], de / e_bf16 [rows, Dt]")
    _lib.call("owl_class_sims_wide_bwd", stream(), dsims, sims, argmax, inv_norm, e, qhat_wide, de, g, e_bf16, rows, Dt, C, Qp)


def query_normalize_wide_bwd(dqhat_wide, queries, dqueries, nq, Dt):
    _chk(dqhat_wide, torch.float32, "dqhat_wide"); _chk(queries, torch.float32, "queries"); _chk(dqueries, torch.float32, "dqueries")
    if dqhat_wide.numel() < 32 * wide_blocks(nq // 3) * Dt:
        raise ValueError("query_normalize_wide_bwd: dqhat_wide must hold [ceil(C / 10) * 32, Dt] floats")
    _lib.call("owl_query_normalize_wide_bwd", stream(), dqhat_wide, queries, dqueries, nq, Dt)


def box_final_bwd(dboxes, sig, h1, u1, w2, du1, partials, dw2_db2, rows, D, du1_colsum=None):
    """partials: f32 [owl_box_final_bwd_blocks(rows), 5 * D + 4]; du1_colsum (optional): += column sums of du1 (dense1's bias gradient)."""
    if partials.numel() < _lib.load().owl_box_final_bwd_blocks(int(rows)) * (5 * int(D) + 4):
        raise ValueError("box_final_bwd: partials must hold owl_box_final_bwd_blocks(rows) x (5 D + 4) floats")
    _chk(du1_colsum, torch.float32, "du1_colsum")
    _lib.call("owl_box_final_bwd", stream(), dboxes, sig, h1, u1, w2, du1, partials, dw2_db2, rows, D, du1_colsum)


# ---- OWLv2's objectness head, its tail (csrc/objectness.hip) ----
def objectness_final(h, w2, b2, logits, rows, D):
    """logits[r] = h[r] . w2 + b2: h bf16 [>= rows, D], w2 f32 [D], b2 f32 one element, logits f32 with at least `rows` elements (written in place)."""
    _chk(h, torch.bfloat16, "h"); _chk(w2, torch.float32, "w2"); _chk(b2, torch.float32, "b2"); _chk(logits, torch.float32, "logits")
    rows, D = int(rows), int(D)
    if h.numel() < rows * D or w2.numel() != D or b2.numel() != 1 or logits.numel() < rows:
        raise ValueError(f"objectness_final: h must hold [{rows}, {D}], w2 [{D}], b2 one element, logits {rows} elements")
    _lib.call("owl_objectness_final_fwd", stream(), h, w2, b2, logits, rows, D)
    return logits


def objectness_final_bwd_blocks(rows):
    return int(_lib.load().owl_objectness_final_bwd_blocks(int(rows)))


def objectness_final_bwd(dlogits, h1, u1, w2, du1, partials, dw2_db2, rows, D, du1_colsum=None):
    """The tail's backward (include/owl_hip.h owl_objectness_final_bwd): dlogits f32 [rows]; h1 / u1 / du1 bf16 [>= rows, D]; partials f32 with
    objectness_final_bwd_blocks(rows) x (2 D + 4) elements; dw2_db2 f32 [D + 4] = dw2, db2, three zeros; du1_colsum (optional) f32 [D].  Outputs are written,
    not accumulated into."""
    _chk(dlogits, torch.float32, "dlogits"); _chk(h1, torch.bfloat16, "h1"); _chk(u1, torch.bfloat16, "u1"); _chk(w2, torch.float32, "w2")
    _chk(du1, torch.bfloat16, "du1"); _chk(partials, torch.float32, "partials"); _chk(dw2_db2, torch.float32, "dw2_db2"); _chk(du1_colsum, torch.float32, "du1_colsum")
    rows, D = int(rows), int(D)
    if dlogits.numel() < rows or min(h1.numel(), u1.numel(), du1.numel()) < rows * D or w2.numel() != D:
        raise ValueError(f"objectness_final_bwd: dlogits must hold {rows} elements, h1 / u1 / du1 [{rows}, {D}], w2 [{D}]")
    if partials.numel() < objectness_final_bwd_blocks(rows) * (2 * D + 4):
        raise ValueError("objectness_final_bwd: partials must hold owl_objectness_final_bwd_blocks(rows) x (2 D + 4) floats")
    if dw2_db2.numel() < D + 4 or (du1_colsum is not None and du1_colsum.numel() < D):
        raise ValueError(f"objectness_final_bwd: dw2_db2 must hold {D + 4} floats (dw2, db2, three zeros), du1_colsum {D}")
    _lib.call("owl_objectness_final_bwd", stream(), dlogits, h1, u1, w2, du1, partials, dw2_db2, rows, D, du1_colsum)


# ---- the box head's dX GEMMs on the rows that carry a gradient (csrc/box_rows_bwd.hip) ----
def box_rows_cap_pad(cap: int) -> int:
    """Rows of the compact operands for a bound of `cap` non-zero rows: the next multiple of 8."""
    return (max(int(cap), 1) + 7) // 8 * 8


def box_rows_state_ints(rows: int) -> int:
    """int32 elements of the compaction's `count_flag`: (count, overflow flag) + one count per workgroup of owl_box_rows_compact."""
    return 2 + _lib.load().owl_box_rows_compact_blocks(int(rows))


def box_rows_compact(dboxes, rows, cap, row_list, count_flag):
    """row_list int32 [>= cap] = ascending indices of the rows of dboxes f32 [rows, 4] with a component that is not == 0; count_flag int32
    [box_rows_state_ints(rows)] = (rows listed, 1 if more than cap were non-zero, then the compaction's scratch).  No host sync."""
    _chk(dboxes, torch.float32, "dboxes"); _chk(row_list, torch.int32, "row_list"); _chk(count_flag, torch.int32, "count_flag")
    rows, cap = int(rows), int(cap)
    if dboxes.numel() < 4 * rows or row_list.numel() < cap or count_flag.numel() < box_rows_state_ints(rows):
        raise ValueError("box_rows_compact: dboxes [rows, 4], row_list [>= cap], count_flag [box_rows_state_ints(rows)]")
    _lib.call("owl_box_rows_compact", stream(), dboxes, rows, cap, row_list, count_flag)


def box_rows_put(pairs, row_list, count_flag, rows, cap, D):
    """pairs: one or two (src bf16 [>= cap, D] or None, dst bf16 [>= rows, D]): dst[row_list[i]] = src[i] for i < count -- zeros where src is None."""
    rows, cap, D = int(rows), int(cap), int(D)
    if not 1 <= len(pairs) <= 2:
        raise ValueError("box_rows_put: one or two (source, destination) pairs")
    for src, dst in pairs:
        _chk(src, torch.bfloat16, "src"); _chk(dst, torch.bfloat16, "dst")
        if dst is None or dst.numel() < rows * D or dst.shape[-1] != D or (src is not None and (src.numel() < cap * D or src.shape[-1] != D)):
            raise ValueError("box_rows_put: src [>= cap, D] or None, dst [>= rows, D]")
    _chk(row_list, torch.int32, "row_list"); _chk(count_flag, torch.int32, "count_flag")
    pairs = list(pairs) + [(None, None)] * (2 - len(pairs))
    _lib.call("owl_box_rows_put", stream(), pairs[0][0], pairs[1][0], pairs[0][1], pairs[1][1], row_list, count_flag, rows, cap, D)


def box_rows_gather(pairs, row_list, count_flag, rows, cap_pad, D):
    """pairs: up to three (src bf16 [>= rows, D], dst bf16 [>= cap_pad, D]): dst[i] = src[row_list[i]] for i < count, zero rows up to cap_pad.  One launch."""
    pairs = [p for p in pairs if p is not None]
    rows, cap_pad, D = int(rows), int(cap_pad), int(D)
    if not 1 <= len(pairs) <= 3:
        raise ValueError("box_rows_gather: one to three (source, destination) pairs")
    for src, dst in pairs:
        _chk(src, torch.bfloat16, "src"); _chk(dst, torch.bfloat16, "dst")
        if src.numel() < rows * D or dst.numel() < cap_pad * D or src.shape[-1] != D or dst.shape[-1] != D:
            raise ValueError("box_rows_gather: src [>= rows, D], dst [>= cap_pad, D]")
    _chk(row_list, torch.int32, "row_list"); _chk(count_flag, torch.int32, "count_flag")
    pairs = pairs + [(None, None)] * (3 - len(pairs))
    _lib.call("owl_box_rows_gather", stream(), pairs[0][0], pairs[1][0], pairs[2][0], pairs[0][1], pairs[1][1], pairs[2][1], row_list, count_flag, rows, cap_pad, D)


def box_rows_scatter_add(dfc, dfeats, row_list, count_flag, rows, cap, D):
    """dfeats f32 [>= rows, D] row row_list[i] += dfc f32 [>= cap, D] row i for i < count."""
    _chk(dfc, torch.float32, "dfc"); _chk(dfeats, torch.float32, "dfeats"); _chk(row_list, torch.int32, "row_list"); _chk(count_flag, torch.int32, "count_flag")
    rows, cap, D = int(rows), int(cap), int(D)
    if dfc.numel() < cap * D or dfeats.numel() < rows * D:
        raise ValueError("box_rows_scatter_add: dfc [>= cap, D], dfeats [>= rows, D]")
    _lib.call("owl_box_rows_scatter_add", stream(), dfc, dfeats, row_list, count_flag, rows, cap, D)


def transpose_colsum(src, dst, colsum, R, C, ld_in=None, ld_out=None, partials=None):
    part = _part(partials, R, C, src.device) if colsum is not None else None
    _lib.call("owl_transpose_colsum_bf16", stream(), src, ld_in if ld_in is not None else src.shape[-1], dst,
              (ld_out if ld_out is not None else dst.shape[-1]) if dst is not None else 0, colsum, R, C,
              part, part.numel() if part is not None else 0)


def colsum_f32(src, colsum, R, C, partials=None):
    part = _part(partials, R, C, src.device)
    _lib.call("owl_colsum_f32", stream(), src, colsum, R, C, part, part.numel())


def embed_bwd(dx, dpos, dcls, dE, B, T, Tp, D):
    """Backward of the embeddings: dpos [T, D] += sum_b dx[b, t], dcls [D] += sum_b dx[b, 0], dE [B (T - 1), D] = bf16 patch rows of dx (no class / pad rows)."""
    _chk(dx, torch.float32, "dx"); _chk(dpos, torch.float32, "dpos"); _chk(dcls, torch.float32, "dcls"); _chk(dE, torch.bfloat16, "dE")
    if dx.numel() < B * Tp * D or dpos.numel() < T * D or dcls.numel() < D or dE.numel() < B * (T - 1) * D:
        raise ValueError("embed_bwd: dx must hold [B, Tp, D], dpos [T, D], dcls [D], dE [B (T - 1), D]")
    _lib.call("owl_embed_bwd", stream(), dx, dpos, dcls, dE, B, T, Tp, D)


def pos_resample(pos, out, g0, g, D):
    """out [g g + 1, D] = the native position table pos [g0 g0 + 1, D] at grid g: class row copied, patch rows bicubic (align_corners=False, A = -0.75, clamped
    taps -- include/owl_hip.h)."""
    _chk(pos, torch.float32, "pos"); _chk(out, torch.float32, "out")
    if pos.numel() < (g0 * g0 + 1) * D or out.numel() < (g * g + 1) * D:
        raise ValueError("pos_resample: pos must hold [g0 g0 + 1, D], out [g g + 1, D]")
    _lib.call("owl_pos_resample", stream(), pos, out, g0, g, D)
    return out


def pos_resample_bwd(dU, dpos, g0, g, D):
    """The adjoint of pos_resample: dpos [g0 g0 + 1, D] += K^T dU [g g + 1, D] (a gather over source cells: no atomics, bitwise reproducible)."""
    _chk(dU, torch.float32, "dU"); _chk(dpos, torch.float32, "dpos")
    if dU.numel() < (g * g + 1) * D or dpos.numel() < (g0 * g0 + 1) * D:
        raise ValueError("pos_resample_bwd: dU must hold [g g + 1, D], dpos [g0 g0 + 1, D]")
    _lib.call("owl_pos_resample_bwd", stream(), dU, dpos, g0, g, D)


def pos_resample_hw(pos, out, g0, gh, gw, D):
    """pos_resample onto a rectangular grid: out [gh gw + 1, D], row 1 + y gw + x (HF's interpolate(size=(gh, gw)); gh == gw is pos_resample, bit for bit)."""
    _chk(pos, torch.float32, "pos"); _chk(out, torch.float32, "out")
    if pos.numel() < (g0 * g0 + 1) * D or out.numel() < (gh * gw + 1) * D:
        raise ValueError("pos_resample_hw: pos must hold [g0 g0 + 1, D], out [gh gw + 1, D]")
    _lib.call("owl_pos_resample_hw", stream(), pos, out, g0, gh, gw, D)
    return out


def pos_resample_bwd_hw(dU, dpos, g0, gh, gw, D):
    """The adjoint of pos_resample_hw: dpos [g0 g0 + 1, D] += K^T dU [gh gw + 1, D]."""
    _chk(dU, torch.float32, "dU"); _chk(dpos, torch.float32, "dpos")
    if dU.numel() < (gh * gw + 1) * D or dpos.numel() < (g0 * g0 + 1) * D:
        raise ValueError("pos_resample_bwd_hw: dU must hold [gh gw + 1, D], dpos [g0 g0 + 1, D]")
    _lib.call("owl_pos_resample_bwd_hw", stream(), dU, dpos, g0, gh, gw, D)


def im2row_bf16(image, out, B, S, ps):
    """out [>= B (S / ps)^2, ld] bf16 <- patches of image [B, 3, S, S] bf16, columns in the conv weight's (c, i, j) order; columns past 3 ps^2 are left alone."""
    _chk(image, torch.bfloat16, "image"); _chk(out, torch.bfloat16, "out")
    if image.numel() < B * 3 * S * S or out.dim() != 2 or out.shape[0] < B * (S // ps) ** 2:
        raise ValueError("im2row_bf16: image must hold [B, 3, S, S], out [>= B (S / ps)^2, ld]")
    _lib.call("owl_im2row_bf16", stream(), image, out, out.shape[1], B, S, ps)


def im2row_bf16_hw(image, out, B, H, W, ps):
    """im2row_bf16 on an image [B, 3, H, W]: out [>= B (H / ps) (W / ps), ld], row (b gh + gy) gw + gx."""
    _chk(image, torch.bfloat16, "image"); _chk(out, torch.bfloat16, "out")
    if image.numel() < B * 3 * H * W or out.dim() != 2 or out.shape[0] < B * (H // ps) * (W // ps):
        raise ValueError("im2row_bf16_hw: image must hold [B, 3, H, W], out [>= B (H / ps) (W / ps), ld]")
    _lib.call("owl_im2row_bf16_hw", stream(), image, out, out.shape[1], B, H, W, ps)


def attention_bwd(qkv, dO, O, lse, dvec, dqkv, B, H, T, Tp, scale, phases=0):
    """phases: 0 = dvec + dK / dV + dQ on this stream; a mask (1 | 2 | 4) launches a subset (dK / dV and dQ only share inputs: tools/attn_bwd_overlap_ab.py)."""
    _lib.call("owl_attention_bwd_bf16", stream(), qkv, dO, O, lse, dvec, dqkv, B, H, T, Tp, float(scale), int(phases))


_pp_ws = {}


NMS_ROUTES = {"per_class": 0, "coordinate_offset": 1, "torchvision_gpu": 2, "torchvision_cpu": 3}


def postprocess(boxes, sims, max_out, conf_thr, iou_thr, route="torchvision_gpu"):
    """owl_postprocess: boxes [B,P,4] f32, sims [B,P,C] f32 -> (boxes [B,K,4], classes [B,K] i64 (-1 pad), scores [B,K]
    (0 pad), patch [B,K] i64 (-1 pad), counts [B] i32) with K = max_out.  ref src/models.py:127-146."""
    B, P, C = sims.shape
    dev = sims.device
    key = (B, P, dev)
    if key not in _pp_ws:
        nbytes = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_postprocess_workspace", B, P, nbytes)
        _pp_ws[key] = torch.empty(int(nbytes.item()), dtype=torch.uint8, device=dev)
    ws = _pp_ws[key]
    out_boxes = torch.zeros(B, max_out, 4, dtype=torch.float32, device=dev)
    out_scores = torch.zeros(B, max_out, dtype=torch.float32, device=dev)
    out_classes = torch.full((B, max_out), -1, dtype=torch.int64, device=dev)
    out_patch = torch.full((B, max_out), -1, dtype=torch.int64, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.call("owl_postprocess", stream(), boxes, sims, ws, ws.numel(), out_boxes, out_scores, out_classes, out_patch, counts,
              B, P, C, max_out, conf_thr, iou_thr, NMS_ROUTES[route])
    return out_boxes, out_classes, out_scores, out_patch, counts


_sm_ws = {}

MERGE_METRICS = {"iou": 0, "ios": 1}
SLICE_MERGE_MAX = 8192     # candidates per source image: the ceiling of the merge's LDS sort and of its scan's 128 mask words


def slice_merge(boxes, scores, classes, counts, xform, slice_offsets, n_groups, n_max, max_out, thr, metric, class_aware):
    """owl_slice_merge: boxes [T,K,4] f32, scores [T,K] f32, classes [T,K] i64, counts [T] i32 (= postprocess' outputs on T slices), xform [T,4] f32 rows
    (sx, ox, sy, oy), slice_offsets [G+1] i32 (a CSR over the G source images), all on the device; n_max >= K * the largest slice count of a group;
    metric 0 | "iou", 1 | "ios" -> (boxes [G,M,4] in full-image coordinates, classes [G,M] i64 (-1 pad), scores [G,M] (0 pad), src [G,M] i64 (-1 pad;
    candidate index: src // K is the slice within its group, src % K the rank in it), counts [G] i32) with M = max_out."""
    _chk(boxes, torch.float32, "boxes"); _chk(scores, torch.float32, "scores"); _chk(classes, torch.int64, "classes"); _chk(counts, torch.int32, "counts")
    _chk(xform, torch.float32, "xform"); _chk(slice_offsets, torch.int32, "slice_offsets")
    if boxes.dim() != 3 or boxes.shape[-1] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]) or tuple(classes.shape) != tuple(scores.shape):
        raise ValueError(f"slice_merge: expected boxes [T,K,4], scores / classes [T,K], got {tuple(boxes.shape)} / {tuple(scores.shape)} / {tuple(classes.shape)}")
    T, K = scores.shape
    G, N, max_out = int(n_groups), int(n_max), int(max_out)
    if tuple(counts.shape) != (T,) or tuple(xform.shape) != (T, 4) or tuple(slice_offsets.shape) != (G + 1,):
        raise ValueError(f"slice_merge: expected counts [{T}], xform [{T},4], slice_offsets [{G + 1}], got {tuple(counts.shape)} / {tuple(xform.shape)} / {tuple(slice_offsets.shape)}")
    dev = boxes.device
    key = (G, N, dev)
    if key not in _sm_ws:
        nbytes = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_slice_merge_workspace", G, N, nbytes)
        _sm_ws[key] = torch.empty(int(nbytes.item()), dtype=torch.uint8, device=dev)
    ws = _sm_ws[key]
    out_boxes = torch.zeros(G, max_out, 4, dtype=torch.float32, device=dev)
    out_scores = torch.zeros(G, max_out, dtype=torch.float32, device=dev)
    out_classes = torch.full((G, max_out), -1, dtype=torch.int64, device=dev)
    out_src = torch.full((G, max_out), -1, dtype=torch.int64, device=dev)
    out_counts = torch.zeros(G, dtype=torch.int32, device=dev)
    _lib.call("owl_slice_merge", stream(), boxes, scores, classes, counts, xform, slice_offsets, ws, ws.numel(), out_boxes, out_scores, out_classes,
              out_src, out_counts, T, K, G, N, max_out, float(thr), int(MERGE_METRICS.get(metric, metric)), 1 if class_aware else 0)
    return out_boxes, out_classes, out_scores, out_src, out_counts


# ---- COCO bbox mAP of the eval loop (csrc/metrics.hip).  The protocol's constants are made ONCE on the host, exactly as pycocotools makes them,
# and handed to the kernels as arrays: device code never re-derives a threshold.
MAP_T, MAP_R, MAP_A, MAP_M = 10, 101, 4, 3
_map_consts = {}


def map_constants(dev):
    """-> dict of device tensors: iou_thr f64 [10], rec_thr f64 [101], area_rng f64 [4,2] (all / small / medium / large), max_dets i32 [3]; eps (float)."""
    dev = torch.device(dev)
    if dev not in _map_consts:
        import numpy as np
        _map_consts[dev] = dict(
            iou_thr=torch.from_numpy(np.linspace(0.5, 0.95, 10)).to(dev), rec_thr=torch.from_numpy(np.linspace(0.0, 1.0, 101)).to(dev),
            area_rng=torch.tensor([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]], dtype=torch.float64, device=dev),
            max_dets=torch.tensor([1, 10, 100], dtype=torch.int32, device=dev), eps=float(np.spacing(1)))
    return _map_consts[dev]


def map_match(det_boxes, det_scores, det_labels, det_counts, gt_boxes, gt_labels, gt_counts, scale, n_classes):
    """owl_map_match: one launch, no host sync.  det_boxes [B,K,4] f32 xyxy, det_scores [B,K] f32, det_labels [B,K] i64 (-1 pad), det_counts [B] i32,
    gt_boxes [B,G,4], gt_labels [B,G] i64, gt_counts [B] i32, scale [B,2] f32 -> (score [B,K], label [B,K] i64 (-1: no record), rank [B,K] i32,
    mask [B,K,4] i32 (bit t matched, bit 10 + t ignored, per area range), npig [B,C,4] i32)."""
    _chk(det_boxes, torch.float32, "det_boxes"); _chk(det_scores, torch.float32, "det_scores"); _chk(det_labels, torch.int64, "det_labels")
    _chk(det_counts, torch.int32, "det_counts"); _chk(gt_boxes, torch.float32, "gt_boxes"); _chk(gt_labels, torch.int64, "gt_labels")
    _chk(gt_counts, torch.int32, "gt_counts"); _chk(scale, torch.float32, "scale")
    B, K = det_scores.shape
    G = gt_labels.shape[1]
    if det_boxes.shape != (B, K, 4) or det_labels.shape != (B, K) or det_counts.shape != (B,) or gt_boxes.shape != (B, G, 4) \
            or gt_labels.shape != (B, G) or gt_counts.shape != (B,) or scale.shape != (B, 2):
        raise ValueError(f"map_match: inconsistent shapes {tuple(det_boxes.shape)} {tuple(det_scores.shape)} {tuple(det_labels.shape)} {tuple(det_counts.shape)} "
                         f"{tuple(gt_boxes.shape)} {tuple(gt_labels.shape)} {tuple(gt_counts.shape)} {tuple(scale.shape)}")
    dev, C = det_scores.device, int(n_classes)
    k = map_constants(dev)
    score = torch.empty(B, K, dtype=torch.float32, device=dev)
    label = torch.empty(B, K, dtype=torch.int64, device=dev)
    rank = torch.empty(B, K, dtype=torch.int32, device=dev)
    mask = torch.empty(B, K, MAP_A, dtype=torch.int32, device=dev)
    npig = torch.empty(B, max(C, 0), MAP_A, dtype=torch.int32, device=dev)
    _lib.call("owl_map_match", stream(), det_boxes, det_scores, det_labels, det_counts, gt_boxes, gt_labels, gt_counts, scale, k["iou_thr"], k["area_rng"],
              score, label, rank, mask, npig, B, K, G, C)
    return score, label, rank, mask, npig


def map_accumulate(rank, mask, seg, npig, n_classes):
    """owl_map_accumulate: rank [N] i32 / mask [N,4] i32 = the records ordered by class, then by descending score (stable); seg [C+1] i64 class
    boundaries; npig [C,4] i32 -> (precision [10,101,C,4,3] f64, recall [10,C,4,3] f64), -1 where a (class, area range) has no ground truth."""
    _chk(rank, torch.int32, "rank"); _chk(mask, torch.int32, "mask"); _chk(seg, torch.int64, "seg"); _chk(npig, torch.int32, "npig")
    C, N = int(n_classes), rank.shape[0]
    if mask.shape != (N, MAP_A) or seg.shape != (C + 1,) or npig.shape != (C, MAP_A):
        raise ValueError(f"map_accumulate: inconsistent shapes {tuple(rank.shape)} {tuple(mask.shape)} {tuple(seg.shape)} {tuple(npig.shape)} for C={C}")
    dev = seg.device
    k = map_constants(dev)
    precision = torch.empty(MAP_T, MAP_R, C, MAP_A, MAP_M, dtype=torch.float64, device=dev)
    recall = torch.empty(MAP_T, C, MAP_A, MAP_M, dtype=torch.float64, device=dev)
    _lib.call("owl_map_accumulate", stream(), rank, mask, seg, npig, k["rec_thr"], k["max_dets"], k["eps"], precision, recall, N, C)
    return precision, recall


_zero_row = {}


def gemm_tn_slab(dy, x, slab, rows, n_out, n_in, splits, variant=0, bias_slab=None):
    """slab[s][n][k] = sum_{m in split s} dy[m][n] * x[m][k] (weight gradient, no transposed copies) -> splits used.
    bias_slab (optional, f32 [>= splits, n_out]): also bias_slab[s][n] = sum_{m in split s} dy[m][n] from the same pass (the bias gradient's partial sums)."""
    _chk(dy, torch.bfloat16, "dy"); _chk(x, torch.bfloat16, "x"); _chk(slab, torch.float32, "slab"); _chk(bias_slab, torch.float32, "bias_slab")
    dev = dy.device
    if dev not in _zero_row:
        _zero_row[dev] = torch.zeros(512, dtype=torch.bfloat16, device=dev)
    used = torch.zeros(1, dtype=torch.int32)
    _lib.call("owl_gemm_tn_slab_bf16", stream(), dy, dy.shape[-1], x, x.shape[-1], _zero_row[dev], slab, rows, n_out, n_in,
              int(splits), used, int(variant), bias_slab)
    return int(used.item())


def colsum_bf16(src, colsum, rows, cols, partials=None):
    _chk(src, torch.bfloat16, "src"); _chk(colsum, torch.float32, "colsum")
    part = _part(partials, rows, cols, src.device)
    _lib.call("owl_colsum_bf16", stream(), src, src.shape[-1], colsum, rows, cols, part, part.numel())


# ---- query bank from image exemplars (csrc/image_query.hip): initialisation-time, outside every step ----
def image_query_workspace_bytes(N, P, Dt) -> int:
    """Bytes of device scratch image_query_select needs (the f64 column-sum partials); a host query, no device call."""
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_image_query_workspace_bytes", N, P, Dt, nbytes)
    return int(nbytes.item())


def image_query_select(e, boxes, qbox, N, P, Dt, diagnostics=False):
    """HF's `embed_image_query` selection per exemplar (include/owl_hip.h): e f32 [>= N P, Dt] (the class head's un-normalised dense0 output), boxes f32
    [N, P, 4] corners, qbox f32 [N, 4] corners or None (= the whole image).  -> (best i32 [N] (-1 = empty), query f32 [N, Dt] = e[n, best] bit for bit,
    info i32 [N, 2] = (flags: bit 0 fallback, bit 1 empty; number selected)); with diagnostics=True also (v f32 [N, P], mean f64 [N, Dt], sim f64 [N, P]).
    No host sync."""
    _chk(e, torch.float32, "e"); _chk(boxes, torch.float32, "boxes"); _chk(qbox, torch.float32, "qbox")
    if e.numel() < N * P * Dt or boxes.numel() < N * P * 4 or (qbox is not None and qbox.numel() != N * 4):
        raise ValueError("image_query_select: e must hold [N, P, Dt], boxes [N, P, 4], qbox [N, 4]")
    dev = e.device
    ws = torch.empty(image_query_workspace_bytes(N, P, Dt), dtype=torch.uint8, device=dev)
    best = torch.empty(N, dtype=torch.int32, device=dev)
    query = torch.empty(N, Dt, dtype=torch.float32, device=dev)
    info = torch.empty(N, 2, dtype=torch.int32, device=dev)
    diag = (torch.empty(N, P, dtype=torch.float32, device=dev), torch.empty(N, Dt, dtype=torch.float64, device=dev),
            torch.empty(N, P, dtype=torch.float64, device=dev)) if diagnostics else (None, None, None)
    _lib.call("owl_image_query_select", stream(), e, boxes, qbox, N, P, Dt, ws, ws.numel(), best, query, info, *diag)
    return (best, query, info) + (diag if diagnostics else ())


def query_bank_fill(query, row_ptr, members, bank, N, nq, Dt):
    """bank [nq, Dt] f32, in place: every row r with members <- unit(sum over members[row_ptr[r] : row_ptr[r + 1]], ascending, of unit(query_m)); rows
    without members keep their bits.  row_ptr i32 [nq + 1] and members i32 are device tensors (models.slots_csr builds them on the host)."""
    _chk(query, torch.float32, "query"); _chk(row_ptr, torch.int32, "row_ptr"); _chk(members, torch.int32, "members"); _chk(bank, torch.float32, "bank")
    if query.numel() < N * Dt or row_ptr.numel() != nq + 1 or bank.numel() < nq * Dt or members.numel() < 1:
        raise ValueError("query_bank_fill: query must hold [N, Dt], row_ptr [nq + 1], bank [nq, Dt], members at least one index")
    _lib.call("owl_query_bank_fill", stream(), query, row_ptr, members, bank, N, nq, Dt)
