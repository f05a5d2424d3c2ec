"""The autograd edge of the HIP train path: ONE coarse torch.autograd.Function around the whole vision
model.  forward = OwlViT._forward_impl (saving the activations of the layers the backward crosses); backward = a
sequence of hand-written HIP kernels (csrc/backward.hip, attention_bwd.hip, gemm.hip) laid out at construction for the
model's trainable set -- by default that of the reference freeze rule (ref src/models.py:173-184): queries, encoder
layer 11, post_layernorm, post_post_layernorm, class_predictor.dense0, box_head.  The dX chain walks from the heads down
to the model's `backward_floor` and stops there (ref main.py:90): an encoder layer on the way is either trained (dX + dW)
or crossed (dX only); below layer 0 lie pre_layernorm and the embeddings.

Parameter gradients are ACCUMULATED by the kernels directly into `model.flat_grad` (each parameter's
.grad is a view of that bucket), so `loss.backward()` leaves one contiguous buffer ready for the single
all-reduce + optimizer step; the Function therefore returns no per-parameter tensors.
"""
from collections import namedtuple

import torch

from . import _lib, ops


DW_ITEMS = 256             # (tile, split) work items a weight-gradient GEMM is cut into: one per CU (bench.py --dw-items: fewer = less slab traffic and CUs left to the dX chain; measured, profiles/r06_tail.md)
TN_SMALL_N = True          # weight-gradient products with at most 64 output rows (the 32 x Dt prompt gradient) on the TN kernel too; False = explicit transposes + NT split-K (A/B)
FOLD_BIAS_COLSUM = True    # bias gradients of the TN-kernel Linears come out of the dW GEMM's own pass (csrc/gemm_tn.hip); False = the separate colsum_bf16 pass (A/B: bench.py --fold-bias 0)


def _grads_attached(model) -> bool:
    """Every trainable parameter's .grad is its view of model.flat_grad."""
    for n, off in model.flat_offsets.items():
        g = model._byname[n].grad
        if g is None or g.data_ptr() != model.flat_grad.data_ptr() + 4 * off:
            return False
    return True


def _attach_grads(model):
    """Make every trainable parameter's .grad a view of model.flat_grad.  If an optimizer set them to
    None (zero_grad(set_to_none=True)) the bucket is zeroed first -- None means zero.  (Callers with a deferred tail order the
    current stream behind it first: optim.FusedAdamW._attach.)"""
    if _grads_attached(model):
        return
    keep = {}
    for n in model.flat_offsets:
        g = model._byname[n].grad
        if g is not None:
            keep[n] = g
    model.flat_grad.zero_()
    for n, off in model.flat_offsets.items():
        p = model._byname[n]
        view = model.flat_grad[off: off + p.numel()].view(p.shape)
        if n in keep and keep[n].data_ptr() != view.data_ptr():
            view.copy_(keep[n])          # foreign accumulated grads are preserved
        p.grad = view


class OwlViTFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, image, image_ids, *params):
        """image_ids: None, or the checked id list of the frozen-prefix cache (models.OwlViT.forward); `image` may then be None."""
        boxes, sims = model._forward_impl(image, save=True, ids=image_ids)
        ctx.model = model
        ctx.B = image.shape[0] if image_ids is None else len(image_ids)
        ctx.sims = sims
        ctx.gen = model._workspace(ctx.B)["gen"]
        return boxes, sims

    @staticmethod
    def backward(ctx, d_boxes, d_sims):
        model, B = ctx.model, ctx.B
        if model._workspace(B)["gen"] != ctx.gen:
            # saved activations live in per-batch-size workspaces (not in ctx): a later gradient-recording forward at this batch
            # size has overwritten them (e.g. two forwards, then (l1 + l2).backward())
            raise RuntimeError(
                f"OwlViT backward: the activations of this forward (batch size {B}) were overwritten by a later gradient-recording "
                "forward at the same batch size (or evicted: only the model's `max_cached_batch_sizes` most recent batch sizes keep their "
                "workspaces); call backward() before the next training forward (no-grad / eval forwards are fine)")
        if getattr(model, "overlap_tail", False) and d_boxes.is_cuda:
            # deferred tail (models.OwlViT.overlap_tail): the whole backward goes to the tail stream; the compute stream carries on with whatever
            # the caller enqueues next (the next forward's frozen prefix) and waits for the event where it touches a trainable tensor
            main, ts = torch.cuda.current_stream(), model._tail_stream
            ts.wait_stream(main)
            for t in (d_boxes, d_sims, ctx.sims):
                t.record_stream(ts)               # (allocated on the compute stream, read on the tail stream)
            with torch.cuda.stream(ts):
                backward_impl(model, B, d_boxes, d_sims, ctx.sims)
                ev = torch.cuda.Event()
                ev.record(ts)
            model._param_event = ev
        else:
            backward_impl(model, B, d_boxes, d_sims, ctx.sims)
        return (None, None, None) + (None,) * len(model.flat_offsets)


class OwlViTQueryFunction(torch.autograd.Function):
    """models.OwlViT.forward_queries with grad enabled: the same forward, HF's class head (ops.class_logits) over the caller's per-image queries on the
    training workspace's e / feats, and backward_impl with the class-head adjoint switched to ops.class_logits_bwd.  The learnable bank takes no part;
    `query_embeds` receives its gradient as an ordinary autograd gradient when it requires one, and so do the four leaves of a trainable logit head
    (models.OwlViT.set_logit_head(head, trainable=True)): they follow the bucket's parameters as explicit inputs, in weights.LOGIT_HEAD_KEYS' order."""

    @staticmethod
    def forward(ctx, model, image, query_embeds, query_mask, *params):
        boxes, _ = model._forward_impl(image, save=True)
        B = image.shape[0]
        logits = model._class_logits_on(model._workspace(B), B, query_embeds, query_mask)
        ctx.model, ctx.B = model, B
        ctx.gen = model._workspace(B)["gen"]
        ctx.qe, ctx.qm = query_embeds.detach(), query_mask
        ctx.n_head = len(params) - len(model.flat_offsets)          # 4: a trainable logit head's leaves; 0: the frozen head, today's launches
        return boxes, logits

    @staticmethod
    def backward(ctx, d_boxes, d_logits):
        model, B = ctx.model, ctx.B
        if model._workspace(B)["gen"] != ctx.gen:
            raise RuntimeError(
                f"OwlViT backward: the activations of this forward (batch size {B}) were overwritten by a later gradient-recording "
                "forward at the same batch size (or evicted: only the model's `max_cached_batch_sizes` most recent batch sizes keep their "
                "workspaces); call backward() before the next training forward (no-grad / eval forwards are fine)")
        dq = torch.empty_like(ctx.qe) if ctx.needs_input_grad[2] else None
        D, nflat = model.cfg.hidden, len(model.flat_offsets)
        dhead = None
        if ctx.n_head and any(ctx.needs_input_grad[4 + nflat:]):
            dhead = torch.empty(2 * D + 2, dtype=torch.float32, device=d_logits.device)          # w_shift | w_scale | b_shift | b_scale
        head = dict(dlogits=d_logits, queries=ctx.qe, mask=ctx.qm, dq=dq, dhead=dhead, event=None)
        if getattr(model, "overlap_tail", False) and d_boxes.is_cuda:
            main, ts = torch.cuda.current_stream(), model._tail_stream
            ts.wait_stream(main)
            for t in (d_boxes, d_logits, ctx.qe, ctx.qm, dq, dhead):
                if t is not None:
                    t.record_stream(ts)           # (allocated on the compute stream, used on the tail stream)
            with torch.cuda.stream(ts):
                if dq is not None or dhead is not None:
                    head["event"] = torch.cuda.Event()          # recorded where the query and logit-head gradients are complete, not at the tail's end
                backward_impl(model, B, d_boxes, None, None, logit_head=head)
                ev = torch.cuda.Event()
                ev.record(ts)
            model._param_event = ev
            if head["event"] is not None:
                main.wait_event(head["event"])    # the query and logit-head gradients go back to the caller's stream: ordered here
        else:
            backward_impl(model, B, d_boxes, None, None, logit_head=head)
        hg = (None,) * ctx.n_head
        if dhead is not None:          # (weights.LOGIT_HEAD_KEYS' order: shift.weight, shift.bias, scale.weight, scale.bias)
            hg = (dhead[:D], dhead[2 * D:2 * D + 1], dhead[D:2 * D], dhead[2 * D + 1:])
        return (None, None, dq, None) + (None,) * nflat + hg


class OwlViTObjectnessFunction(torch.autograd.Function):
    """OWLv2's objectness head with a TRAINABLE head (models.OwlViT.set_objectness_head(head, trainable=True)), called by forward_queries(..., objectness=True)
    right behind the recording forward: o = dense2(gelu(dense1(gelu(dense0(feats))))) on the training workspace's feats, read as a constant (HF detaches
    them: there is no dX into the trunk).  Inputs: the six leaves in weights.OBJECTNESS_HEAD_KEYS' order.  backward returns views of ONE flat f32 gradient
    (the layout of the head's parameter buffer), written, not accumulated into.  It shares no scratch with backward_impl -- activations, du1 / du0, the
    tail's partials, the transposed weight and the weight-gradient scratch are its own (_objectness_bws) -- and runs on the caller's stream, so it may
    run before, after or without the main backward, in line or beside the deferred tail, with the same bits; model.flat_grad is not touched."""

    @staticmethod
    def forward(ctx, model, B, *leaves):
        out = model._objectness_train_forward(B)
        ctx.model, ctx.B = model, B
        ctx.gen = model._workspace(B)["gen"]
        return out

    @staticmethod
    def backward(ctx, d_obj):
        model, B = ctx.model, ctx.B
        if model._workspace(B)["gen"] != ctx.gen or ("obj", B) not in model._ws:
            raise RuntimeError(
                f"OwlViT backward: the activations of this forward (batch size {B}) were overwritten by a later gradient-recording "
                "forward at the same batch size (or evicted: only the model's `max_cached_batch_sizes` most recent batch sizes keep their "
                "workspaces); call backward() before the next training forward (no-grad / eval forwards are fine)")
        if not any(ctx.needs_input_grad[2:]):
            return (None,) * 8
        cfg = model.cfg
        D, Mh = cfg.hidden, B * cfg.patches
        ws, ow, bw = model._workspace(B), model._objectness_ws(B), _objectness_bws(model, B)
        oh, at = model.objectness_head, model._objectness_layout()[0]
        g = torch.zeros(model._objectness_layout()[1], dtype=torch.float32, device=d_obj.device)          # (dense0's bias gradient is added into: it starts at zero)
        view = lambda k: g[at[k][0]:at[k][1]].view(at[k][2])
        d = d_obj.contiguous().float().view(-1)
        a2 = at["dense2.weight"][0]
        ops.objectness_final_bwd(d, ow["h1"], ow["u1"], oh["dense2.weight"].detach(), bw["du1"], bw["part"], g[a2:a2 + D + 4], Mh, D,
                                 du1_colsum=view("dense1.bias"))
        weight_grad(bw["du1"], ow["h0"], view("dense1.weight"), D, D, Mh, bw["dw"], accumulate=0)
        ops.transpose_bf16(model._objectness_bf16["dense1.weight"], bw["w1T"], D, D)
        ops.gemm(ops.EPI_DGELU_BF16, bw["du1"], bw["w1T"], bw["du0"], aux=ow["u0"], M=Mh, N=D, K=D)
        weight_grad(bw["du0"], ws["feats"], view("dense0.weight"), D, D, Mh, bw["dw"], view("dense0.bias"), accumulate=0)
        from . import weights as W
        return (None, None) + tuple(view(k) for k in W.OBJECTNESS_HEAD_KEYS)


def _objectness_bws(model, B):
    """Backward scratch of the objectness head at this batch size, allocated when its first backward runs: du1 / du0 bf16 [B P, D], the tail's partials, the
    bf16 transpose of dense1.weight and a weight_grad scratch of its own (nothing of _bws(): the main backward may be running beside this one)."""
    key = ("obj_bwd", B)
    if key in model._ws:
        return model._ws[key]
    D, Mh, dev = model.cfg.hidden, B * model.cfg.patches, model.device_
    bf, z = torch.bfloat16, ops.zeros_rows
    dw = dw_scratch(D, D, Mh, dev, bias=True)          # (both products are D x D; dense0's carries the bias gradient)
    bw = dict(du1=z(Mh, D, bf, dev), du0=z(Mh, D, bf, dev), part=torch.zeros(ops.objectness_final_bwd_blocks(Mh), 2 * D + 4, device=dev),
              w1T=torch.zeros(D, D, dtype=bf, device=dev), dw=dw)
    model._ws[key] = bw
    return bw


def _bws(model, B):
    key = ("bwd", B)
    if key in model._ws:
        return model._ws[key]
    cfg, dev = model.cfg, model.device_
    D, I, Tp, P, Dt, H = cfg.hidden, cfg.mlp, cfg.tokens_padded, cfg.patches, cfg.text_dim, cfg.heads
    M, Mh = B * Tp, B * P
    Mp, Mhp = ops.pad_rows(M), ops.pad_rows(Mh)
    bf, f32 = torch.bfloat16, torch.float32
    z = ops.zeros_rows
    Qg = _routed_cols(model)                                 # columns of the routed upstream G = rows of dqhat: 32, or the wide head's Qp
    sz = _dw_sizes(cfg, Qg, model._train_emb)
    ws = dict(
        de=z(Mh, Dt, bf, dev), dqhat=torch.zeros(Qg, Dt, device=dev),
        # (du1 / du0 / box_part, the [Mh, D] workspaces of a DENSE box-head backward, are made when one first runs: _box_dense_ws; the row path's: _box_rows_ws)
        g32=z(Mh, Qg, bf, dev), e_bf=z(Mh, Dt, bf, dev),
        slab=torch.zeros(sz.slab, device=dev),
        sink=torch.zeros(4 * D + 8, device=dev),          # where kernels that must run leave the gradients of FROZEN tensors (never read; not in the bucket)
        # per-split partial sums of the bias gradients (one row of n_out floats per split of the dW GEMM; at most 256 splits); the class head's chain has its own
        bslab=torch.zeros(256 * max(3 * D, I, Dt), device=dev), bslab2=torch.zeros(256 * max(D, Dt), device=dev),
        dfeats=z(Mh, D, f32, dev), dcls=torch.zeros(B, D, device=dev),
        dx=z(M, D, f32, dev), dxb=z(M, D, bf, dev), du=z(M, I, bf, dev), dh=z(M, D, bf, dev), dxm=z(M, D, f32, dev),
        datt=z(M, D, bf, dev), dqkv=z(M, 3 * D, bf, dev),
        dvec=torch.zeros(B, H, Tp, device=dev),
        # partial sums of the deterministic row reductions (bias / LayerNorm-affine gradients): written by one kernel, added in a
        # fixed order by the next -- no f32 atomics into the gradient bucket
        part=ops.rowreduce_workspace(B, Tp, max(3 * D, I, Dt), dev),
        part2=ops.rowreduce_workspace(B, Tp, max(3 * D, I, Dt), dev),      # ... of the weight-gradient stream (see backward_impl)
        dxb2=z(M, D, bf, dev),                                              # second bf16 dx of the trainable layer (the first one is still being read)
        # transposed-operand scratch for the dW GEMMs; token-row and head-row users get their own buffers so
        # that the zero pad columns [rows, rows_pad) of each are never dirtied by the other row count
        # (only the products _dw_plan() sends down the NT route need them: the parity-test configs' and the 32 x Dt prompt-gradient product; the
        #  patch-embedding weight gradient, where embeddings train, shares the head-row pair)
        tA=torch.zeros(sz.tok_rows, Mp, dtype=bf, device=dev) if sz.tok_rows else None,
        tB=torch.zeros(sz.tok_rows, Mp, dtype=bf, device=dev) if sz.tok_rows else None,
        tAh=torch.zeros(sz.tAh_rows, Mhp, dtype=bf, device=dev),
        tBh=torch.zeros(sz.tBh_rows, Mhp, dtype=bf, device=dev),
        wT=torch.zeros(max(3 * D, I) * max(D, I), dtype=bf, device=dev),
        # the class head's backward runs beside the box head's on the side stream: its own split-K slab and transposed-weight scratch
        slab2=torch.zeros(sz.slab2, device=dev),
        wT2=torch.zeros(Dt * D, dtype=bf, device=dev),
        tn_all=sz.tn_all,
    )
    # the scratch of one weight-gradient launch (weight_grad), by who launches it -- the same buffers, no memory of their own:
    # this stream at head rows (the heads, the patch embedding); the class head where it runs on the side stream; the encoder layers' weight-gradient stream
    ws["dw_main"] = dict(slab=ws["slab"], part=ws["part"], bslab=ws["bslab"], tA=ws["tAh"], tB=ws["tBh"], tn_all=sz.tn_all)
    ws["dw_class"] = dict(slab=ws["slab2"], part=ws["part2"], bslab=ws["bslab2"], tA=ws["tAh"], tB=ws["tBh"], tn_all=sz.tn_all)
    ws["dw_enc"] = dict(slab=ws["slab"], part=ws["part2"], bslab=ws["bslab"], tA=ws["tA"], tB=ws["tB"], tn_all=sz.tn_all)
    model._ws[key] = ws
    return ws


def _box_dense_ws(model, B, bw, du0=True):
    """du1 (and du0) bf16 [Mh, D] and the tail's partials of the box-head backward, allocated when first needed at this batch size: the row path reads du1
    alone, so a run whose box gradients all come marked from the criterion never makes the 113 MB du0."""
    D, Mh, dev = model.cfg.hidden, B * model.cfg.patches, model.device_
    if "du1" not in bw:
        bw["du1"] = ops.zeros_rows(Mh, D, torch.bfloat16, dev)
        bw["box_part"] = torch.zeros(_lib.load().owl_box_final_bwd_blocks(Mh), 5 * D + 4, device=dev)
    if du0 and "du0" not in bw:
        bw["du0"] = ops.zeros_rows(Mh, D, torch.bfloat16, dev)
    return bw


def _box_rows_ws(model, B, bw, cap_pad):
    """The row path's workspaces at this batch size, grown to the largest bound seen: the row list and (count, overflow flag) and the compact operands
    [pad_rows(cap_pad), D] (rows beyond cap_pad stay zero: never written).  Where the box head trains, also du0z: a dense bf16 [Mh, D] buffer that is all
    zero between backwards (the listed rows of du0 are put in for dense0's weight-gradient product and cleared after it)."""
    rw = bw.get("box_rows")
    if rw is None or rw["cap_pad"] < cap_pad:
        D, dev = model.cfg.hidden, model.device_
        bf, z = torch.bfloat16, ops.zeros_rows
        rw = dict(cap_pad=cap_pad, row_list=torch.zeros(cap_pad, dtype=torch.int32, device=dev),
                  count_flag=torch.zeros(ops.box_rows_state_ints(B * model.cfg.patches), dtype=torch.int32, device=dev),
                  du1c=z(cap_pad, D, bf, dev), du0c=z(cap_pad, D, bf, dev), ub0c=z(cap_pad, D, bf, dev), dfc=z(cap_pad, D, torch.float32, dev),
                  du0z=None if rw is None else rw["du0z"])
        bw["box_rows"] = rw
    if "box_head" in model._units and rw["du0z"] is None:
        rw["du0z"] = ops.zeros_rows(B * model.cfg.patches, model.cfg.hidden, torch.bfloat16, model.device_)
    return rw


BOX_ROWS_MARK = "_owl_box_rows_cap"          # attribute the criteria put on the box gradient they return: at most that many rows of it are non-zero


def mark_box_rows(d_boxes, cap):
    """The promise of a criterion whose box loss reads the matched predictions only (losses._PushPullFn / _OpenVocabFn): at most `cap` rows of the
    [B, P, 4] gradient it returns are non-zero.  backward_impl then runs the box head's dX GEMMs on those rows.  A broken promise is loud, not wrong: more
    than `cap` non-zero rows turn dense0's gradients and d(feats) into NaN (csrc/box_rows_bwd.hip)."""
    setattr(d_boxes, BOX_ROWS_MARK, int(cap))
    return d_boxes


def _box_rows_cap(model, d_boxes, B, P):
    """The bound of a marked box gradient the row path takes, or None: the dense launches."""
    cap = getattr(d_boxes, BOX_ROWS_MARK, None)
    if cap is None or getattr(model, "box_backward", "auto") != "auto":
        return None
    if d_boxes.dtype != torch.float32 or not d_boxes.is_contiguous() or tuple(d_boxes.shape) != (B, P, 4):
        return None
    if ops.box_rows_cap_pad(cap) * 8 > B * P:          # (tiny configs with many targets: nothing to gain)
        return None
    return int(cap)


def _split_k(n_rows_out, n_cols_out, k):
    """Split the (long) token contraction so that a dW GEMM gives every CU about one work item.  A work-item heuristic of its own: `t` is NOT the
    library's tile rule (gemm_plan.h, gemm_auto_big, also wants 48 tiles of 256 x 256), and the split counts, hence gradient bits and slab sizes, rest
    on this arithmetic as it stands."""
    t = 256 if (n_rows_out >= 512 and n_cols_out >= 256) else 128
    tiles = ((n_rows_out + t - 1) // t) * ((n_cols_out + t - 1) // t)
    slots = 256 if t == 256 else 512
    return max(1, min(k // 64, slots // tiles))


def _qkv_grads(model, i):
    """f32 [3D, D] and [3D] views of the bucket: the gradients of trainable layer i's fused q / k / v weight (models.OwlViT._wqkv) and bias."""
    D, pre = model.cfg.hidden, f"backbone.encoder.layers.{i}.self_attn.q_proj."
    o, ob = model.flat_offsets[pre + "weight"], model.flat_offsets[pre + "bias"]
    return model.flat_grad[o: o + 3 * D * D].view(3 * D, D), model.flat_grad[ob: ob + 3 * D]


def _routed_cols(model):
    """Columns of the class head's routed upstream G (= rows of dqhat): one 32-column tile, or the wide head's Qp (a multiple of 256)."""
    return ops.wide_qp(model.cfg.n_classes) if model.wide_head else 32


DwPlan = namedtuple("DwPlan", "tn splits n_in_pad slab_elems")
DwSizes = namedtuple("DwSizes", "tn_all slab slab2 tok_rows tAh_rows tBh_rows")


def _dw_plan(n_out, n_in, *, bias=False, tn_all=False, rows=None):
    """How one weight-gradient product grad_w[n_out, n_in] (+)= dy[rows, n_out]^T x[rows, n_in] is launched (weight_grad) -- the one place that decides it.
    tn: the TN kernel (csrc/gemm_tn.hip) reads dy / x where they lie.  It takes the products whose two sides are multiples of 256, and -- TN_SMALL_N -- one
      with at most 64 output rows (a multiple of 8: one 256-wide n tile of which those rows are kept; the 32 x Dt prompt gradient, 92 us -> ~30,
      profiles/r06_tail.md) where every token-row product is on the kernel too (`tn_all`) and no bias gradient rides along (`bias`).  Every other product:
      two explicit transposes, then the NT split-K GEMM over n_in padded to a multiple of 8 (`n_in_pad`; L/14's 588 patch columns run as 592).
    splits: the split count to request -- DW_ITEMS (at most 256, one per CU) work items over the TN kernel's 256 x 256 tiles, or _split_k() of the NT
      kernel's own tiles at `rows` (None: at any row count).  The kernels may use fewer, never more.
    slab_elems: f32 elements the split-K slabs of that route can take at any row count and any DW_ITEMS (the scratch outlives a change of the switch)."""
    if n_in % 256 == 0 and (n_out % 256 == 0 or (TN_SMALL_N and n_out % 8 == 0 and n_out <= 64 and tn_all and not bias)):
        tiles = ((n_out + 255) // 256) * (n_in // 256)
        return DwPlan(True, max(1, min(DW_ITEMS, 256) // tiles), n_in, max(1, 256 // tiles) * n_out * n_in)
    n_in_pad = (n_in + 7) // 8 * 8
    most = _split_k(n_out, n_in_pad, 1 << 30)
    return DwPlan(False, most if rows is None else _split_k(n_out, n_in_pad, ops.pad_rows(rows)), n_in_pad, most * n_out * n_in_pad)


def _dw_sizes(cfg, routed_cols=32, train_emb=False):
    """Scratch of backward_impl's weight-gradient launches, from _dw_plan() of every product it can launch (no device, no tensor) -> tn_all: every product of
    the encoder's and the class head's widths is on the TN kernel; f32 elements of the split-K slab and of the class-head lane's own; rows of the token-row
    transposed-operand pair tA / tB (0: none) and of the head-row pair (tAh holds dy^T: n_out rows, tBh holds x^T: n_in rows)."""
    D, I, Dt = cfg.hidden, cfg.mlp, cfg.text_dim
    plan = lambda n_out, n_in, tn_all=False: (n_out, n_in, _dw_plan(n_out, n_in, tn_all=tn_all))          # (a bias gradient bears on the small-n_out exception alone: the routed product, which has none)
    enc = [plan(3 * D, D), plan(D, D), plan(I, D), plan(D, I)]          # token rows
    tn_all = all(p.tn for _, _, p in enc + [plan(Dt, D)])
    # head rows: the class head's products, which run on either lane (the routed one with and without the small-n_out exception: TN_SMALL_N may flip after
    # the workspaces exist), the box head's and the patch embedding's
    cls = [plan(Dt, D), plan(routed_cols, Dt, tn_all), plan(routed_cols, Dt)]
    head = cls + [plan(D, D)] + ([plan(D, cfg.patch_k)] if train_emb else [])
    nt = [(n_out, n_in) for n_out, n_in, p in head if not p.tn]
    # (floors: the head widths, or one 32-row tile where every token-row product is on the TN kernel; what the NT products need only ever raises them)
    return DwSizes(tn_all, slab=max(p.slab_elems for _, _, p in enc + head), slab2=max(p.slab_elems for _, _, p in cls),
                   tok_rows=0 if tn_all else max(max(n_out, n_in) for n_out, n_in, _ in enc),
                   tAh_rows=max([32 if tn_all else max(D, Dt)] + [n_out for n_out, _ in nt]), tBh_rows=max([D, Dt] + [n_in for _, n_in in nt]))


def weight_grad(dy, x, grad_w, n_out, n_in, rows, scratch, grad_b=None, accumulate=1):
    """grad_w[n_out, n_in] (+)= dy[rows, n_out]^T x[rows, n_in];  grad_b += colsum(dy), on the route _dw_plan() picks: split-K GEMM into f32 slabs ->
    deterministic slab reduction.  dy [>= rows, n_out] and x [>= rows, ld >= n_in] bf16.
    scratch: dict(slab; with a bias gradient also part, bslab; for the NT route tA [>= n_out, pad_rows(rows)], tB [>= n_in, pad_rows(rows)]; tn_all) --
    one of _bws()'s three.  Pad columns [rows, pad_rows(rows)) of tA / tB stay zero: never written, buffers start zeroed."""
    plan = _dw_plan(n_out, n_in, bias=grad_b is not None, tn_all=scratch.get("tn_all", False), rows=rows)
    slab = scratch["slab"]
    if plan.tn:
        # no token-major copies (LDS transpose-reads).  The bias gradient (column sums of dy) comes out of the same pass as per-split partial sums and is
        # added up like the weight slabs
        bs = scratch["bslab"] if (grad_b is not None and FOLD_BIAS_COLSUM) else None
        if grad_b is not None and bs is None:          # (A/B switch off: the column-sum kernel)
            ops.colsum_bf16(dy, grad_b, rows, n_out, partials=scratch["part"])
        ns = ops.gemm_tn_slab(dy, x, slab, rows, n_out, n_in, plan.splits, bias_slab=bs)
        _lib.call("owl_slab_reduce", ops.stream(), slab, grad_w, n_out * n_in, n_out * n_in, ns, accumulate)
        if bs is not None:
            _lib.call("owl_slab_reduce", ops.stream(), bs, grad_b, n_out, n_out, ns, 1)
        return
    tA, tB = scratch["tA"], scratch["tB"]
    ld, Kp = ops.pad_rows(rows), plan.n_in_pad
    assert tA.shape[1] == ld and tB.shape[1] == ld and tA.shape[0] >= n_out and tB.shape[0] >= n_in
    ops.transpose_colsum(dy, tA, grad_b, rows, n_out, ld_in=dy.shape[-1], ld_out=ld, partials=scratch.get("part"))
    ops.transpose_colsum(x, tB, None, rows, n_in, ld_in=x.shape[-1], ld_out=ld)
    ns = _lib.load().owl_gemm_effective_splits(ld, plan.splits)
    # (rows [n_in, Kp) of the W operand do not exist: w_rows clamps the loads, and the row-by-row reducer leaves those columns of the slabs alone)
    ops.gemm(ops.EPI_SLAB_F32, tA, tB, slab, M=n_out, N=Kp, K=ld, lda=ld, ldw=ld, ldo=Kp, a_rows=n_out, w_rows=n_in, splits=plan.splits)
    if Kp == n_in:
        _lib.call("owl_slab_reduce", ops.stream(), slab, grad_w, n_out * n_in, n_out * n_in, ns, accumulate)
    else:
        _lib.call("owl_slab_reduce_rows", ops.stream(), slab, grad_w, n_out, n_in, Kp, n_out * Kp, ns, accumulate)


def dw_scratch(n_out, n_in, rows, device, bias=False):
    """A weight_grad() scratch of its own for one product shape at `rows` rows, for callers outside backward_impl's three lanes: the split-K slab, the
    NT route's transposed-operand pair where _dw_plan() takes that route and, with a bias gradient, the per-split bias slab (256 splits at most) and the
    column reduction's partials."""
    plan, ld, bf = _dw_plan(n_out, n_in, bias=bias), ops.pad_rows(rows), torch.bfloat16
    scratch = dict(slab=torch.zeros(plan.slab_elems, device=device), tn_all=False,
                   tA=None if plan.tn else torch.zeros(n_out, ld, dtype=bf, device=device), tB=None if plan.tn else torch.zeros(n_in, ld, dtype=bf, device=device))
    if bias:
        scratch.update(bslab=torch.zeros(256 * n_out, device=device), part=torch.zeros(ops.part_floats(rows, n_out), device=device))
    return scratch


def patch_weight_grad(dE, patches, grad_w, D, K, rows, scratch=None, accumulate=1):
    """grad_w [D, K] (+)= dE[rows, D]^T patches[rows, K] -- the patch-embedding weight gradient: weight_grad() without a bias (scratch as there; default:
    allocated here)."""
    if scratch is None:
        scratch = dw_scratch(D, K, rows, dE.device)
    weight_grad(dE, patches, grad_w, D, K, rows, scratch, accumulate=accumulate)


def backward_impl(model, B, d_boxes, d_sims, sims, logit_head=None):
    """logit_head (None = the bank head's adjoint, today's launches): dict(dlogits [B, P, Q], queries, mask, dq, dhead, event) -- the class-head section is then
    the adjoint of ops.class_logits (OwlViTQueryFunction): class_logits_bwd writes de and the shift / scale part of d(feats), dense0's dW runs as ever,
    its dX GEMM ACCUMULATES into d(feats), then the box head's does: one fixed order of the three contributions.  `dq` (or None) receives the query
    gradient, `dhead` (or None: a frozen logit head, today's launches) the f32 [2 D + 2] gradients of logit_shift / logit_scale -- two more launches in
    the class-head section, on its stream, also where the floor forms no d(feats) -- and `event` (or None) is recorded on the calling stream once both
    are complete.  d_sims / sims are not read."""
    cfg = model.cfg
    D, I, H, Tp, T, P, Dt, C = cfg.hidden, cfg.mlp, cfg.heads, cfg.tokens_padded, cfg.tokens, cfg.patches, cfg.text_dim, cfg.n_classes
    M, Mh = B * Tp, B * P
    ws, bw = model._workspace(B), _bws(model, B)
    P_ = model._byname
    model._wait_params()
    model._grad_clean = False
    _attach_grads(model)
    G = lambda n: P_[n].grad                      # views into model.flat_grad (accumulated into)
    tv = model._tview
    units, tls, floor, low = model._units, model._tl_set, model.backward_floor, model._chain_low
    t_q, t_cls, t_box = "queries" in units, "class_predictor.dense0" in units, "box_head" in units
    below_heads = floor != "heads"                # the dX chain goes on below feats
    below_enc = floor in ("pre_layernorm", "embeddings")
    LP = lambda i: f"backbone.encoder.layers.{i}."
    if getattr(model, "box_backward", "auto") not in ("auto", "dense"):
        raise ValueError(f"model.box_backward must be 'auto' or 'dense', got {model.box_backward!r}")
    box_cap = _box_rows_cap(model, d_boxes, B, P)          # (read off the tensor autograd handed over: a copy below would not carry the mark)
    d_boxes = d_boxes.contiguous().float()
    if logit_head is None:
        d_sims = d_sims.contiguous().float()
    else:
        d_logits = logit_head["dlogits"].contiguous().float()

    # the forward launched the transposes on their own stream (models.OwlViT._pretranspose_weights): order this stream behind them once
    pre_wt = model._wt if (getattr(model, "pretranspose", False) and model._wt_event is not None) else None
    if pre_wt is not None:
        torch.cuda.current_stream().wait_event(model._wt_event)

    def wT(name, rows, cols, buf=bw["wT"]):
        """bf16 transpose of a weight [rows, cols] -> [cols, rows].  Trainable: the forward's pre-transposed copy, or (pretranspose off) made here in scratch;
        frozen but crossed by the dX chain: the static copy made at construction."""
        if name not in model.flat_offsets:
            return model._fz[name + ".T"]
        if pre_wt is not None:
            return pre_wt[name]
        out = buf[: rows * cols].view(cols, rows)
        ops.transpose_bf16(tv(name), out, rows, cols)
        return out

    # The two heads only meet in d(feats): with sub-batch streams on (and every dW on the TN kernel, so that the heads share no transposed-operand
    # scratch) the class head's backward runs on the side stream with its own slab / reduction / transposed-weight scratch, beside the box
    # head's on this one; the box head's last GEMM accumulates into d(feats) behind the class head's event.  Same kernels, same order of the
    # two contributions: same bits.
    # (streams: in-line, the backward shares the forward's side streams; as a deferred tail -- models.OwlViT.overlap_tail -- it has side streams
    #  and fork / join events of its own, because the next forward is using the model's while this runs)
    # A frozen head unit launches no dW; where the dX chain stops at the heads (floor "heads") nothing below e / feats runs for it either, and a head
    # that neither trains nor is crossed does not run at all.
    S, J, fork = model._bwd_streams()
    main0 = torch.cuda.current_stream()
    hs = S(1) if (model.head_streams and model.encoder_streams > 1 and len(model._encoder_chunks(B)) > 1 and bw["tn_all"]) else main0
    ev_h = model._dw_events
    if hs is not main0:
        ev_h[0].record(main0)
        hs.wait_event(ev_h[0])
    cdw, cw = (bw["dw_class"], bw["wT2"]) if hs is not main0 else (bw["dw_main"], bw["wT"])
    # ---- class head ---------------------------------------------------------------------------------
    with torch.cuda.stream(hs):
        if logit_head is not None:
            # HF's class head over the caller's queries (csrc/open_vocab_bwd.hip); the learnable bank takes no part
            dq, dhead = logit_head["dq"], logit_head.get("dhead")
            if t_cls or below_heads or dq is not None or dhead is not None:
                lh, qe, qm = model.logit_head, logit_head["queries"], logit_head["mask"]
                nbanks = B if qe.dim() == 3 else 1
                if dhead is None:
                    key, need, more = "ovb", ops.class_logits_bwd_workspace_bytes(B, P, qe.shape[-2], nbanks, Dt, dq is not None), {}
                else:          # the head trains: the same launches, the row pass also stores (dshift, ds) per row, two more launches reduce them
                    key, need = "ovb", ops.class_logits_bwd_head_workspace_bytes(B, P, qe.shape[-2], nbanks, Dt, D, dq is not None)
                    if "ovb_rowgrad" not in bw:
                        bw["ovb_rowgrad"] = torch.zeros(Mh, 2, dtype=torch.float32, device=model.device_)
                    more = dict(feats=ws["feats"], dhead=dhead, rowgrad=bw["ovb_rowgrad"])
                if key not in bw or bw[key].numel() < need:          # (one buffer per batch size, grown to the largest query count seen)
                    bw[key] = torch.empty(need, dtype=torch.uint8, device=model.device_)
                ops.class_logits_bwd(d_logits, ws["e"], qe, lh["logit_shift.weight"].detach(), lh["logit_scale.weight"].detach(), ws["logit_rowstats"], B, P,
                                     mask=qm, de=bw["de"], dfeats=bw["dfeats"] if below_heads else False, dqueries=dq if dq is not None else False,
                                     workspace=bw[key], **more)
                if t_cls:
                    weight_grad(bw["de"], ws["feats"], G("class_predictor.dense0.weight"), Dt, D, Mh, cdw, G("class_predictor.dense0.bias"))
                if below_heads:
                    ops.gemm(ops.EPI_ACC_F32, bw["de"], wT("class_predictor.dense0.weight", Dt, D, buf=cw), bw["dfeats"], M=Mh, N=D, K=Dt)
        elif t_q or t_cls or below_heads:
            if model.wide_head:          # label sets beyond 10 classes: de as a dense f32-MFMA product, G [rows, Qp] in the wide query layout (csrc/class_head_wide.hip)
                Qp = bw["g32"].shape[1]
                ops.class_sims_wide_bwd(d_sims, sims, ws["argmax"], ws["inv_norm"], ws["e"], ws["qhat"], bw["de"], bw["g32"], bw["e_bf"], Mh, Dt, C)
                if t_q:
                    weight_grad(bw["g32"], bw["e_bf"], bw["dqhat"], Qp, Dt, Mh, cdw, accumulate=0)          # dqhat = G^T e
                    ops.query_normalize_wide_bwd(bw["dqhat"], P_["queries"], G("queries"), cfg.queries, Dt)
            else:
                ops.class_sims_bwd(d_sims, sims, ws["argmax"], ws["inv_norm"], ws["e"], ws["qhat"], bw["de"], bw["g32"], bw["e_bf"], Mh, Dt, C)
                if t_q:
                    weight_grad(bw["g32"], bw["e_bf"], bw["dqhat"], 32, Dt, Mh, cdw, accumulate=0)          # dqhat = G^T e
                    _lib.call("owl_query_normalize_bwd", ops.stream(), bw["dqhat"], P_["queries"], G("queries"), cfg.queries, Dt)
            if t_cls:
                weight_grad(bw["de"], ws["feats"], G("class_predictor.dense0.weight"), Dt, D, Mh, cdw, G("class_predictor.dense0.bias"))
            if below_heads:
                ops.gemm(ops.EPI_F32, bw["de"], wT("class_predictor.dense0.weight", Dt, D, buf=cw), bw["dfeats"], M=Mh, N=D, K=Dt)
        if hs is not main0:
            ev_h[1].record(hs)
    # ---- box head -------------------------------------------------------------------------------------
    # A box gradient that comes marked from the criterion (mark_box_rows: at most `cap` non-zero rows) runs the section's two dX GEMMs -- du0 through the
    # erf-GELU' and the product into d(feats): 340 of the section's 660 us at B/16 batch 32 -- on those rows: compaction -> gather -> the GEMMs at M = cap_pad
    # -> scatter-add into d(feats).  Every GEMM row depends on its own A row alone: same bits.  The sums over rows (the tail kernel, the two weight-gradient
    # products) stay the dense launches they were, dense0's on du0z = the listed rows of du0 where they lie in a buffer that is zero elsewhere (a zero row
    # adds exact zeros): every gradient keeps its bits, and a training run its trajectory.
    w0T = rw = None
    if t_box or below_heads:
        model.last_box_backward = "dense" if box_cap is None else "rows"
        _box_dense_ws(model, B, bw, du0=box_cap is None)
        if t_box:
            gw2, gb2 = G("box_head.dense2.weight"), G("box_head.dense2.bias")
            assert gb2.data_ptr() == gw2.data_ptr() + 4 * gw2.numel(), "dense2 weight/bias grads must be adjacent in the flat bucket"
        else:
            gw2 = bw["sink"]          # (the kernel has to run for du1 and takes no null there)
        ops.box_final_bwd(d_boxes, ws["sig"], ws["hb1"], ws["ub1"], P_["box_head.dense2.weight"], bw["du1"], bw["box_part"], gw2, Mh, D,
                          du1_colsum=G("box_head.dense1.bias") if t_box else None)          # (dense1's bias gradient from the same pass: no column-sum launch over du1)
        if t_box:
            weight_grad(bw["du1"], ws["hb0"], G("box_head.dense1.weight"), D, D, Mh, bw["dw_main"])
        if box_cap is not None:
            cap_pad = ops.box_rows_cap_pad(box_cap)
            rw = _box_rows_ws(model, B, bw, cap_pad)
            rl, cf = rw["row_list"], rw["count_flag"]
            ops.box_rows_compact(d_boxes, Mh, box_cap, rl, cf)
            ops.box_rows_gather([(bw["du1"], rw["du1c"]), (ws["ub0"], rw["ub0c"])], rl, cf, Mh, cap_pad, D)
            ops.gemm(ops.EPI_DGELU_BF16, rw["du1c"], wT("box_head.dense1.weight", D, D), rw["du0c"], aux=rw["ub0c"], M=cap_pad, N=D, K=D)
            if t_box:
                ops.box_rows_put([(rw["du0c"], rw["du0z"])], rl, cf, Mh, box_cap, D)
                weight_grad(rw["du0z"], ws["feats"], G("box_head.dense0.weight"), D, D, Mh, bw["dw_main"], G("box_head.dense0.bias"))
                ops.box_rows_put([(None, rw["du0z"])], rl, cf, Mh, box_cap, D)
            if below_heads:
                ops.gemm(ops.EPI_F32, rw["du0c"], wT("box_head.dense0.weight", D, D), rw["dfc"], M=cap_pad, N=D, K=D)
        else:
            ops.gemm(ops.EPI_DGELU_BF16, bw["du1"], wT("box_head.dense1.weight", D, D), bw["du0"], aux=ws["ub0"], M=Mh, N=D, K=D)
            if t_box:
                weight_grad(bw["du0"], ws["feats"], G("box_head.dense0.weight"), D, D, Mh, bw["dw_main"], G("box_head.dense0.bias"))
            if below_heads:
                w0T = wT("box_head.dense0.weight", D, D)
    if hs is not main0:
        main0.wait_event(ev_h[1])                 # d(feats) of the class head is in place (and the side stream's scratch is free again)
    if logit_head is not None and logit_head.get("event") is not None:
        logit_head["event"].record(main0)         # the query gradient is complete on this stream from here on
    if not below_heads:
        return
    if rw is not None:
        ops.box_rows_scatter_add(rw["dfc"], bw["dfeats"], rw["row_list"], rw["count_flag"], Mh, box_cap, D)
    else:
        ops.gemm(ops.EPI_ACC_F32, bw["du0"], w0T, bw["dfeats"], M=Mh, N=D, K=D)
    # ---- merge + the two final LayerNorms --------------------------------------------------------------
    # (the kernel takes no null for the four affine gradients: those of a frozen LayerNorm go to the sink)
    sink = bw["sink"]
    t_pl, t_ppl = "backbone.post_layernorm" in units, "post_post_layernorm" in units
    last = cfg.layers - 1
    ops.merge_ln_bwd(bw["dfeats"], ws["x_fin"], ws["cls_ln"], ws["st_post"], ws["st_pp"], P_["backbone.post_layernorm.weight"],
                     P_["backbone.post_layernorm.bias"], P_["post_post_layernorm.weight"], bw["dx"], bw["dcls"],
                     G("backbone.post_layernorm.weight") if t_pl else sink[:D], G("backbone.post_layernorm.bias") if t_pl else sink[D:2 * D],
                     G("post_post_layernorm.weight") if t_ppl else sink[2 * D:3 * D], G("post_post_layernorm.bias") if t_ppl else sink[3 * D:4 * D],
                     B, P, Tp, D, partials=bw["part"], dx_bf16=bw["dxb"],
                     dx_colsum=G(LP(last) + "mlp.fc2.bias") if last in tls else None)     # (dx here = d(output of the last layer))
    if low is None:
        return
    scale = cfg.head_dim ** -0.5
    # (bw["dxb"] always holds the bf16 copy of bw["dx"]: every kernel that writes dx writes it too -- no separate cast pass)

    def dx_only(layers):
        """A run of frozen layers the chain crosses (e.g. those above layer 11 under the literal "layers.11" rule on a deeper model): dX only.
        Like the encoder forward (models.OwlViT._forward_impl), this chain couples no two images: it runs as sub-batches (row ranges of the
        same buffers) on the model's streams, layer by layer."""
        chunks = model._encoder_chunks(B)
        main = torch.cuda.current_stream()
        streams = [main] + [S(c) for c in range(1, len(chunks))]
        if len(chunks) > 1:
            fork.record(main)
            for s_ in streams[1:]:
                s_.wait_event(fork)
        for i in layers:
            Ls, fz = model._layer_ws(B, i), model._fz
            pre = LP(i)
            for (b0, nb), s_ in zip(chunks, streams):
                r0, Mc = b0 * Tp, nb * Tp
                R = lambda t: t[r0:r0 + Mc]
                with torch.cuda.stream(s_):
                    ops.gemm(ops.EPI_DQGELU_BF16, R(bw["dxb"]), fz[f"{i}.w2T"], R(bw["du"]), aux=R(Ls["gp"]), M=Mc, N=I, K=D, concurrency=len(chunks))
                    ops.gemm(ops.EPI_BIAS_BF16, R(bw["du"]), fz[f"{i}.w1T"], R(bw["dh"]), M=Mc, N=D, K=I, concurrency=len(chunks))
                    # (the LayerNorm backward also writes the bf16 copy of its dx: the operand of the next dX GEMM, no separate cast pass)
                    ops.layernorm_bwd(R(bw["dh"]), R(Ls["x_mid"]), R(Ls["st2"]), P_[pre + "layer_norm2.weight"], R(bw["dx"]), R(bw["dxm"]), None, None,
                                      Mc, D, dx_bf16=R(bw["dxb"]))
                    ops.gemm(ops.EPI_BIAS_BF16, R(bw["dxb"]), fz[f"{i}.woT"], R(bw["datt"]), M=Mc, N=D, K=D, concurrency=len(chunks))
                    ops.attention_bwd(R(Ls["qkv"]), R(bw["datt"]), R(Ls["att"]), Ls["lse"][b0:b0 + nb], bw["dvec"][b0:b0 + nb], R(bw["dqkv"]),
                                      nb, H, T, Tp, scale)
                    ops.gemm(ops.EPI_BIAS_BF16, R(bw["dqkv"]), fz[f"{i}.wqkvT"], R(bw["dh"]), M=Mc, N=D, K=3 * D, concurrency=len(chunks))
                    ops.layernorm_bwd(R(bw["dh"]), R(Ls["x_in"]), R(Ls["st1"]), P_[pre + "layer_norm1.weight"], R(bw["dxm"]), R(bw["dx"]), None, None,
                                      Mc, D, dx_bf16=R(bw["dxb"]))
        for c, s_ in enumerate(streams):
            if c > 0:
                J(c).record(s_)
                main.wait_event(J(c))

    def train(i, fc2_bias_done, goes_on, train_below):
        """Trainable encoder layer i.  fc2_bias_done: the kernel that produced dx already summed its columns into this layer's fc2 bias gradient;
        goes_on: the chain continues below this layer (its LayerNorm 1 backward then also emits dx); train_below: ... into a trainable layer, whose fc2
        bias gradient that kernel sums on the way."""
        # Two chains: dX (this stream) and the four weight gradients.  A weight gradient feeds nothing downstream -- it only has to be in the
        # bucket when backward() returns -- so the dW GEMMs (+ their bias column sums and slab reductions) run on the model's side stream, each
        # behind the event of the dX-chain kernel that produces its operand: its workgroups fill the CUs the dX kernels' last rounds leave
        # idle, and vice versa.  Same kernels on the same operands: same bits.  The side stream owns the split-K slab from here on and has its
        # own reduction scratch; the second bf16 dx goes to its own buffer because dW(fc2) may still be reading the first.  The side stream is
        # in-order: the dW chains of successive trainable layers queue behind each other on the one set of scratch.
        tl, Lt, dwe = LP(i), model._layer_ws(B, i), bw["dw_enc"]
        main = torch.cuda.current_stream()
        side = S(1) if model.encoder_streams > 1 else main
        evs = model._dw_events

        def on_side(k, fn):
            if side is main:
                fn()
                return
            evs[k].record(main)
            side.wait_event(evs[k])
            with torch.cuda.stream(side):
                fn()

        # MLP
        if not fc2_bias_done:     # (the last layer's fc2 bias gradient came out of merge_ln_bwd, that of a layer below a trainable one out of its LayerNorm 1 backward)
            ops.colsum_f32(bw["dx"], G(tl + "mlp.fc2.bias"), M, D, partials=bw["part"])
        on_side(0, lambda: weight_grad(bw["dxb"], Lt["g"], G(tl + "mlp.fc2.weight"), D, I, M, dwe))
        dxc = 1 if side is main else 2          # (the weight-gradient GEMMs run beside the dX chain: ops.gemm's small-problem rule counts them)
        ops.gemm(ops.EPI_DQGELU_BF16, bw["dxb"], wT(tl + "mlp.fc2.weight", D, I), bw["du"], aux=Lt["gp"], M=M, N=I, K=D, concurrency=dxc)
        on_side(1, lambda: weight_grad(bw["du"], Lt["h2"], G(tl + "mlp.fc1.weight"), I, D, M, dwe, G(tl + "mlp.fc1.bias")))
        ops.gemm(ops.EPI_BIAS_BF16, bw["du"], wT(tl + "mlp.fc1.weight", I, D), bw["dh"], M=M, N=D, K=I, concurrency=dxc)
        ops.layernorm_bwd(bw["dh"], Lt["x_mid"], Lt["st2"], P_[tl + "layer_norm2.weight"], bw["dx"], bw["dxm"],
                          G(tl + "layer_norm2.weight"), G(tl + "layer_norm2.bias"), M, D, dx_bf16=bw["dxb2"], partials=bw["part"],
                          dx_colsum=G(tl + "self_attn.out_proj.bias"))     # (dx here = d(x + out-proj output): its column sums are that bias's gradient)
        # attention
        on_side(2, lambda: weight_grad(bw["dxb2"], Lt["att"], G(tl + "self_attn.out_proj.weight"), D, D, M, dwe))
        woT = wT(tl + "self_attn.out_proj.weight", D, D)
        ops.gemm(ops.EPI_BIAS_BF16, bw["dxb2"], woT, bw["datt"], M=M, N=D, K=D, concurrency=dxc)
        ops.attention_bwd(Lt["qkv"], bw["datt"], Lt["att"], Lt["lse"], bw["dvec"], bw["dqkv"], B, H, T, Tp,
                          cfg.head_dim ** -0.5)
        g_wqkv, g_bqkv = _qkv_grads(model, i)
        on_side(3, lambda: weight_grad(bw["dqkv"], Lt["h1"], g_wqkv, 3 * D, D, M, dwe, g_bqkv))
        if pre_wt is not None:
            wqkvT = pre_wt[tl + "qkv"]
        else:
            wqkvT = bw["wT"][: 3 * D * D].view(D, 3 * D)
            ops.transpose_bf16(model._wqkv(i), wqkvT, 3 * D, D)
        ops.gemm(ops.EPI_BIAS_BF16, bw["dqkv"], wqkvT, bw["dh"], M=M, N=D, K=3 * D, concurrency=dxc)
        if not goes_on:
            # everything below layer_norm1 is frozen: only its affine parameters need gradients
            ops.layernorm_bwd(bw["dh"], Lt["x_in"], Lt["st1"], P_[tl + "layer_norm1.weight"], None, None,
                              G(tl + "layer_norm1.weight"), G(tl + "layer_norm1.bias"), M, D, partials=bw["part"])
            if side is not main:
                evs[4].record(side)
                main.wait_event(evs[4])
            return
        # The chain goes on: LayerNorm 1's backward writes the dx / bf16 dx the weight-gradient chain of this layer is still reading (dW(fc2)), and the
        # layer below rewrites du / dxb2 / dqkv -- so the join with the side stream comes first (dW(qkv) has run beside the GEMM above).
        if side is not main:
            evs[4].record(side)
            main.wait_event(evs[4])
        ops.layernorm_bwd(bw["dh"], Lt["x_in"], Lt["st1"], P_[tl + "layer_norm1.weight"], bw["dxm"], bw["dx"],
                          G(tl + "layer_norm1.weight"), G(tl + "layer_norm1.bias"), M, D, dx_bf16=bw["dxb"], partials=bw["part"],
                          dx_colsum=G(LP(i - 1) + "mlp.fc2.bias") if train_below else None)     # (dx here = d(output of layer i - 1))

    # ---- the encoder, from the last layer down to the floor: each layer either trained or crossed ----------------------------------------
    i = last
    while i >= low:
        if i in tls:
            train(i, fc2_bias_done=(i == last or (i + 1) in tls), goes_on=(i > low or below_enc), train_below=(i - 1 >= low and (i - 1) in tls))
            i -= 1
        else:
            run = []
            while i >= low and i not in tls:
                run.append(i)
                i -= 1
            dx_only(run)
    if not below_enc:
        return
    # ---- below layer 0: pre_layernorm and the embeddings (bw["dx"] = d(output of pre_layernorm), f32) ----------------------------------------
    pw = model._pre_ws(B)
    t_pre, t_emb = model._train_pre, model._train_emb
    ops.layernorm_bwd(bw["dx"], pw["x_emb"], pw["st_pre"], P_["backbone.pre_layernorm.weight"], None, bw["dxm"] if t_emb else None,
                      G("backbone.pre_layernorm.weight") if t_pre else None, G("backbone.pre_layernorm.bias") if t_pre else None, M, D, partials=bw["part"])
    if t_emb:
        g_pos = G("backbone.embeddings.position_embedding.weight")
        if model._pos_used is None:
            ops.embed_bwd(bw["dxm"], g_pos, G("backbone.embeddings.class_embedding"), pw["dE"], B, T, Tp, D)
        else:
            # run grid != native grid: the batch sum lands in a zeroed [T, D] scratch (the gradient of the resampled table), and the resampler's adjoint
            # accumulates it into the native-shape gradient; dcls and dE as ever
            dU = pw["dU"]
            dU.zero_()
            ops.embed_bwd(bw["dxm"], dU, G("backbone.embeddings.class_embedding"), pw["dE"], B, T, Tp, D)
            ops.pos_resample_bwd_hw(dU, g_pos, cfg.native_grid, cfg.grid_h, cfg.grid_w, D)
        ops.im2row_bf16_hw(ws["img"], pw["patches"], B, *cfg.image_hw, cfg.patch_size)
        patch_weight_grad(pw["dE"], pw["patches"], G("backbone.embeddings.patch_embedding.weight").view(D, cfg.patch_k), D, cfg.patch_k, Mh, scratch=bw["dw_main"])
