"""OWL-ViT vision path on MI355X -- host-side mirror of reference src/models.py.

Call surface kept from the reference:
    model = load_model(labelmap, device)            # ref src/models.py:149
    pred_boxes, None, pred_sims, None = model(image) # ref src/models.py:98-119
    model.parameters() / .train() / .eval() / named_parameters() with the reference's names, so the
    freeze rule (ref src/models.py:173-184) and `torch.optim.AdamW(model.parameters(), ...)`
    (ref main.py:56-60) work unchanged.

Everything below that surface is new: the forward and backward are sequences of hand-written HIP
kernels (libowlhip.so, C ABI in include/owl_hip.h) driven from one coarse autograd.Function; PyTorch
only owns memory, streams and the autograd edge.  Activations are bf16 with an f32 residual stream;
trainable parameters are f32 views into ONE flat bucket (and their grads into one flat grad bucket,
which is what the single RCCL all-reduce per step operates on -- SURVEY.md section 8e).
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, weights as W
from .config import OwlConfig, check_image_size, get_config, table_grid
from .postprocess import PostProcess  # noqa: F401  (the reference exports it from src/models.py:122)
from .prefix_cache import PrefixCache, _id_list


def box_bias_table(grid: int, grid_w: int = None) -> torch.Tensor:
    """HF5:1071-1104 `compute_box_bias(num_patches_height, num_patches_width)` (computed once on the host, as HF keeps
    it as a buffer): [P,4] f32, p = y*gw + x.  box_bias_table(g) is the square g x g table; box_bias_table(gh, gw) divides x by gw and y by gh and
    biases the width by 1 / gw and the height by 1 / gh."""
    gh, gw = grid, (grid if grid_w is None else grid_w)
    xx, yy = torch.meshgrid(torch.arange(1, gw + 1, dtype=torch.float32), torch.arange(1, gh + 1, dtype=torch.float32), indexing="xy")
    bc = torch.stack((xx, yy), dim=-1)
    bc[..., 0] /= gw
    bc[..., 1] /= gh
    bc = torch.clip(bc.view(-1, 2), 0.0, 1.0)
    coord_bias = torch.log(bc + 1e-4) - torch.log1p(-bc + 1e-4)
    size = torch.full_like(coord_bias, 1.0)
    size[..., 0] /= gw
    size[..., 1] /= gh
    size_bias = torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)
    return torch.cat([coord_bias, size_bias], dim=-1).contiguous()


class _Node(nn.Module):
    """Bare container so that parameter names match the reference module tree."""


_POS = "backbone.embeddings.position_embedding.weight"
_LAYER_ORDER = ([f"self_attn.{p}_proj.weight" for p in "qkv"] + [f"self_attn.{p}_proj.bias" for p in "qkv"]
                + ["self_attn.out_proj.weight", "self_attn.out_proj.bias", "layer_norm1.weight", "layer_norm1.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                   "mlp.fc2.weight", "mlp.fc2.bias", "layer_norm2.weight", "layer_norm2.bias"])
_UNIT_ORDER = {
    "queries": ["queries"],
    "backbone.post_layernorm": ["backbone.post_layernorm.weight", "backbone.post_layernorm.bias"],
    "post_post_layernorm": ["post_post_layernorm.weight", "post_post_layernorm.bias"],
    "class_predictor.dense0": ["class_predictor.dense0.weight", "class_predictor.dense0.bias"],
    "box_head": ["box_head.dense0.weight", "box_head.dense0.bias", "box_head.dense1.weight", "box_head.dense1.bias", "box_head.dense2.weight", "box_head.dense2.bias"],
    "backbone.pre_layernorm": ["backbone.pre_layernorm.weight", "backbone.pre_layernorm.bias"],
    "backbone.embeddings": ["backbone.embeddings.class_embedding", "backbone.embeddings.patch_embedding.weight", "backbone.embeddings.position_embedding.weight"],
}


def _flat_order(cfg: OwlConfig, trainable=None):
    """Order of the trainable tensors inside the flat bucket (q,k,v adjacent -> fused views).  `trainable`: the substring list of the freeze rule (None = the
    reference's).  Units follow weights.BUCKET_UNITS -- queries, the trainable encoder layers in ascending order, post_layernorm, post_post_layernorm, the class
    head, the box head, pre_layernorm, the embeddings -- so the reference set keeps the layout its checkpoints and optimizer states were written with."""
    units, layers = W.trainable_units(cfg, trainable)
    names = []
    for u in W.BUCKET_UNITS:
        if u == "layers":
            for i in layers:
                names += [f"backbone.encoder.layers.{i}." + n for n in _LAYER_ORDER]
        elif u in units:
            names += _UNIT_ORDER[u]
    return names


class OwlViT(nn.Module):
    """Vision-only OWL-ViT with a learnable query bank (ref src/models.py:41-119)."""

    def __init__(self, cfg: OwlConfig, state: "dict[str, np.ndarray]", device="cuda", encoder_streams: int = 2, trainable=None):
        """trainable: None = the reference's freeze rule (weights.FREEZE_KEEP); otherwise an iterable of substrings with the reference's semantics -- a
        parameter is trainable iff any of them occurs in its name ("layers.1" therefore selects layers 1 AND 10 to 19).  The selection must be made of whole
        units (weights.BUCKET_UNITS: queries, class_predictor.dense0, box_head, backbone.post_layernorm, post_post_layernorm, each encoder layer,
        backbone.pre_layernorm, backbone.embeddings); a partial unit or an empty selection raises ValueError.

        cfg.pos_grid (0 = cfg.grid): side of the NATIVE position table.  The parameter `backbone.embeddings.position_embedding.weight` keeps that
        shape [g0 g0 + 1, D] whatever cfg.image_size is, so checkpoints, the flat bucket and optimizer states are interchangeable between input sizes; at
        another run grid the embeddings read a resampled table (ops.pos_resample: bicubic, HF's `interpolate_pos_encoding`) the model owns."""
        super().__init__()
        self.cfg = cfg
        if cfg.pos_grid:
            check_image_size(cfg.image_size, cfg.patch_size, cfg.pos_rows)          # (an int or a pair, as the config holds it)
        self.device_ = torch.device(device)
        if cfg.head_dim != 64:
            raise ValueError("attention kernels are built for head_dim = 64")
        if not 1 <= cfg.n_classes <= ops.WIDE_MAX_CLASSES:
            raise ValueError(f"OwlViT: the class head takes label sets of 1 to {ops.WIDE_MAX_CLASSES} classes (3 prompts each), got {cfg.n_classes}")
        if self.device_.type == "cuda" and torch.cuda.is_available():
            cus = torch.cuda.get_device_properties(self.device_).multi_processor_count
            if cus != ops.CHIP_CUS:
                import warnings
                warnings.warn(f"OwlViT: {self.device_} reports {cus} compute units; the kernels' grids and tile rules are laid out for the {ops.CHIP_CUS} CUs of an "
                              "unpartitioned MI355X (results stay correct, the schedule is not the measured one)")
        shapes = W.param_shapes(cfg)
        missing = set(shapes) - set(state)
        if missing:
            raise KeyError(f"missing parameters: {sorted(missing)[:4]} ...")
        rows = int(np.asarray(state[_POS]).shape[0])
        if rows != cfg.pos_rows:
            raise ValueError(f"OwlViT: the position table in `state` has {rows} rows, the config expects {cfg.pos_rows} (native grid {cfg.native_grid}); "
                             f"build the config with pos_grid={table_grid(rows)}, or let load_model(..., image_size=) infer it")
        self._keep = None if trainable is None else tuple(trainable)
        keep = W.FREEZE_KEEP if self._keep is None else self._keep
        units, self.trainable_layers = W.trainable_units(cfg, self._keep)
        self._units, self._tl_set = frozenset(units), frozenset(self.trainable_layers)
        self.backward_floor = W.backward_floor(units)          # the lowest point the backward's dX chain reaches
        # lowest encoder layer the dX chain crosses (None: the chain ends above the encoder)
        self._chain_low = self.backward_floor if isinstance(self.backward_floor, int) else (0 if self.backward_floor in ("pre_layernorm", "embeddings") else None)
        self._train_emb, self._train_pre = "backbone.embeddings" in units, "backbone.pre_layernorm" in units
        order = _flat_order(cfg, self._keep)
        assert set(order) == {n for n in shapes if W.is_trainable(n, keep)}, "flat order must cover the trainable set"

        # ---- flat trainable bucket (f32) + grad bucket; every tensor starts 8-element aligned ----
        offs, off = OrderedDict(), 0
        for n in order:
            offs[n] = off
            off += (int(np.prod(shapes[n])) + 7) // 8 * 8
        self.flat_numel = off
        self.flat_offsets = offs
        self.flat_param = torch.zeros(off, dtype=torch.float32, device=self.device_)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=self.device_)
        self.flat_bf16 = torch.zeros(off, dtype=torch.bfloat16, device=self.device_)

        # ---- parameter tree with the reference's names ---------------------------------------------
        self._pnames = []
        for name, shape in shapes.items():
            src = torch.as_tensor(np.asarray(state[name]), dtype=torch.float32)
            assert tuple(src.shape) == tuple(shape), name
            if name in offs:
                view = self.flat_param[offs[name]: offs[name] + src.numel()].view(shape)
                view.copy_(src)
                p = nn.Parameter(view, requires_grad=True)
            else:
                p = nn.Parameter(src.to(self.device_), requires_grad=False)
            self._attach(name, p)
            self._pnames.append(name)
        self._byname = dict(self.named_parameters())
        assert list(self._byname.keys()) == list(shapes.keys()) or set(self._byname) == set(shapes)

        # ---- frozen bf16 compute copies ---------------------------------------------------------------
        D = cfg.hidden
        self._fz = {}
        P_ = self._byname
        with torch.no_grad():
            # im2row-free for every patch size (L/14's 14-pixel rows included): the weight goes into the gather loader's K order once (weights.py)
            wpe = W.patch_weight_gather_layout(P_["backbone.embeddings.patch_embedding.weight"].detach(), cfg.patch_size)
            self._pe_gather = None
            if not self._train_emb:
                self._fz["w_pe"] = wpe.to(torch.bfloat16).contiguous()
            elif wpe.shape[1] == cfg.patch_k:
                # trainable, 2^n patch size: the gather order is the parameter's own -> the forward reads the bucket's bf16 copy where it lies
                self._fz["w_pe"] = self._tview("backbone.embeddings.patch_embedding.weight").view(D, cfg.patch_k)
            else:
                # trainable, other patch sizes: a per-step product of the bucket (_refresh_patch_weight), re-laid out by one column gather / scatter; the
                # column map comes from the same function that lays the frozen weight out
                cols = W.patch_weight_gather_layout(np.arange(1, cfg.patch_k + 1, dtype=np.float32)[None, :], cfg.patch_size)[0]
                dst = np.nonzero(cols)[0]
                self._pe_gather = (torch.as_tensor(dst, dtype=torch.int64, device=self.device_),
                                   torch.as_tensor(cols[dst].astype(np.int64) - 1, device=self.device_))
                self._fz["w_pe"] = torch.zeros(D, wpe.shape[1], dtype=torch.bfloat16, device=self.device_)
            for i in range(cfg.layers):
                if i in self._tl_set:
                    continue
                pre = f"backbone.encoder.layers.{i}."
                self._fz[f"{i}.wqkv"] = torch.cat([P_[pre + f"self_attn.{p}_proj.weight"] for p in "qkv"], 0).to(torch.bfloat16).contiguous()
                self._fz[f"{i}.bqkv"] = torch.cat([P_[pre + f"self_attn.{p}_proj.bias"] for p in "qkv"], 0).contiguous()
                self._fz[f"{i}.wo"] = P_[pre + "self_attn.out_proj.weight"].to(torch.bfloat16).contiguous()
                self._fz[f"{i}.w1"] = P_[pre + "mlp.fc1.weight"].to(torch.bfloat16).contiguous()
                self._fz[f"{i}.w2"] = P_[pre + "mlp.fc2.weight"].to(torch.bfloat16).contiguous()
                if self._chain_low is not None and i >= self._chain_low:
                    # frozen layers the backward's dX chain crosses (e.g. those above layer 11 under the literal "layers.11" rule on a deeper
                    # model, ref src/models.py:175): the backward passes through them (dX only) -> static transposed copies
                    for k in ("wqkv", "wo", "w1", "w2"):
                        self._fz[f"{i}.{k}T"] = self._fz[f"{i}.{k}"].t().contiguous()
            # frozen heads: bf16 compute copies of their GEMM weights and, where the dX chain crosses them, the transposed copies -- made once, here
            for n in ("class_predictor.dense0.weight", "box_head.dense0.weight", "box_head.dense1.weight"):
                if n not in offs:
                    self._fz[n] = P_[n].to(torch.bfloat16).contiguous()
                    if self.backward_floor != "heads":
                        self._fz[n + ".T"] = self._fz[n].t().contiguous()
        self.box_bias = box_bias_table(cfg.grid_h, cfg.grid_w).to(self.device_)
        # run grid != native grid: the embeddings read `_pos_used` [T, D], the native table resampled (the parameter keeps its native shape).  Frozen
        # embeddings: made here and after every load_state_dict; trainable ones: by every forward (_forward_impl).  At the native size nothing of this exists.
        self._pos_used = None
        if cfg.resampled:                  # (by the grid's two sides, not by P: 4 x 9 has the 36 patches of a native 6 x 6 table)
            self._pos_used = torch.zeros(cfg.tokens, D, dtype=torch.float32, device=self.device_)
            self._refresh_pos()
            self.register_load_state_dict_post_hook(lambda module, incompatible: module._refresh_pos())
        self._ws = {}
        self._gen = 0                      # generation of the latest forward (any batch size): see _forward_impl / autograd.OwlViTFunction
        self._ws_lru = []                  # batch sizes, most recent first: workspaces of all but the newest `max_cached_batch_sizes` are dropped
        self.max_cached_batch_sizes = 2    # (a DataLoader's ragged last batch + the regular one; every further size would pin its own activations)
        self._saved = None
        # The bf16 compute copy of the trainable bucket is re-cast by EVERY forward -- one pass over 8.7 M elements -- unless the fused AdamW has
        # just written it in its own pass: FusedAdamW.step leaves a ONE-SHOT token (this flag + the bucket's version counter) that the next
        # forward consumes.  Nothing else can set it, so writes the version counter does not see (`p.data.mul_()`, raw-pointer kernels) are picked
        # up by the next forward at the latest one forward after an optimizer step (see refresh_compute_weights for the remaining window).
        self._bf16_current = False
        self._bf16_version = None          # flat_param._version at the fused step that set the token
        self.encoder_streams = int(encoder_streams)     # sub-batches of the encoder forward, one HIP stream each (see _forward_impl); 1 = off
        self._streams, self._join, self._fork_ev, self._fork_ev_tail = [], {}, None, None
        self.head_streams = True          # box head / class head (forward and backward) on two streams when the sub-batch streams are on
        self._dw_events_ = None
        self._param_event = None           # the deferred tail of the previous step (backward / all-reduce / AdamW on the tail stream): see overlap_tail
        self._grad_clean = False           # ... which also left flat_grad zeroed for this step
        # overlap_tail (optim.FusedAdamW(..., overlap=True) / ddp.DataParallel(overlap=True) switch it on): the hand-written backward, the gradient
        # all-reduce and the fused AdamW of step i run on ONE side stream ("tail stream") while the compute stream already runs the forward of step
        # i+1 -- embeddings and encoder layers below the trainable one are frozen (ref src/models.py:173-184), so nothing before the trainable layer
        # depends on the tail; the compute stream waits for it exactly where the first trainable tensor / kept activation is touched (_wait_params).
        # The tail's small kernels (loss backward, head backward, reductions, transposes: ~1 ms at 32 workgroups or fewer) then run beside the next
        # forward's GEMMs instead of alone.  Same kernels, same operands, same order per buffer: bitwise the in-line schedule.
        self.overlap_tail = False
        self._tail_stream_ = None
        # Round 6 experiment, OFF by default: with `pretranspose` the backward's seven weight transposes (bf16 W^T of the trainable weights, the "W" operand of the
        # dX GEMMs; they do not depend on the loss) are launched by a gradient-recording forward on a stream of their own where it first reads the trainable
        # weights, and run beside the trainable layer / heads / loss chain instead of inside the backward.  Same kernels, same operands: same bits
        # (tests/test_determinism_gpu.py).  Measured (profiles/r06_tail.md): 74 us of transposes leave the backward's stream and the step does not get
        # faster (three alternated rounds: +0.17 / -0.38 / -0.23 %): the in-backward form stays the default.
        self.pretranspose = False
        self._wt, self._wt_stream_, self._wt_event = None, None, None
        # box_backward: "auto" = a box gradient that comes marked from the criterion (autograd.mark_box_rows: PushPullLoss / OpenVocabLoss read the matched
        # predictions only, so all but at most B * Nmax rows of it are zero) runs the box head's two dX GEMMs on those rows (csrc/box_rows_bwd.hip; the
        # sums over rows stay dense launches: every gradient bitwise the dense section's); any other gradient takes the dense launches.
        # "dense" = always the dense launches (A/B).  last_box_backward: "rows" | "dense", the path the last backward's box-head section took (None: none ran).
        self.box_backward = "auto"
        self.last_box_backward = None
        self._trainable = frozenset(order)
        # checkpointing while a deferred optimizer step (ddp.DataParallel(overlap=True)) is still running on its side stream: order the
        # current stream behind it before any parameter is read
        self.register_state_dict_pre_hook(lambda module, prefix, keep_vars: module._wait_params())
        # Frozen-prefix activation cache (prefix_cache.py; off until enable_prefix_cache()): with `model(image, image_ids=ids)` the residual stream at the
        # entry of the first non-frozen consumer is kept per id, and the frozen layers below it run on the images not yet kept only.  Whatever may change
        # a frozen tensor empties it.
        self.prefix_cache = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate_prefix())
        # HF's class_head.logit_shift / logit_scale for zero-shot inference (detect): frozen device buffers outside flat_param, the parameter tree and
        # every state dict (plain attributes, as box_bias is); None until set_logit_head
        self.logit_head = None
        self._logit_head_flat = None          # the one buffer behind a TRAINABLE head's four leaf views (set_logit_head(head, trainable=True))
        # OWLv2's objectness head (HF `objectness_head.*`), on the same terms: None until set_objectness_head
        self.objectness_head = None
        self._objectness_flat = None          # the one buffer behind a TRAINABLE head's six leaf views
        self._objectness_bf16 = None          # bf16 copies of dense0.weight / dense1.weight for the GEMMs

    # -- module-tree plumbing -----------------------------------------------------------------------
    def _attach(self, dotted: str, p: nn.Parameter):
        parts = dotted.split(".")
        node = self
        for part in parts[:-1]:
            if part not in node._modules:
                node.add_module(part, _Node())
            node = node._modules[part]
        node.register_parameter(parts[-1], p)

    def p(self, name: str) -> torch.Tensor:
        return self._byname[name]

    def _tview(self, name: str, dtype=torch.bfloat16):
        """bf16 (or f32) view of a trainable tensor inside the flat buckets."""
        o = self.flat_offsets[name]
        n = self._byname[name].numel()
        src = self.flat_bf16 if dtype == torch.bfloat16 else self.flat_param
        return src[o: o + n].view(self._byname[name].shape)

    def _hw(self, name: str):
        """bf16 compute copy of a head GEMM weight: the bucket's view, or the frozen copy."""
        return self._tview(name) if name in self.flat_offsets else self._fz[name]

    def _layer_weights(self, i: int):
        cfg, D = self.cfg, self.cfg.hidden
        pre = f"backbone.encoder.layers.{i}."
        P_ = self._byname
        if i in self._tl_set:
            o = self.flat_offsets[pre + "self_attn.q_proj.weight"]
            wqkv = self.flat_bf16[o: o + 3 * D * D].view(3 * D, D)
            ob = self.flat_offsets[pre + "self_attn.q_proj.bias"]
            bqkv = self.flat_param[ob: ob + 3 * D]
            wo, w1, w2 = (self._tview(pre + "self_attn.out_proj.weight"), self._tview(pre + "mlp.fc1.weight"),
                          self._tview(pre + "mlp.fc2.weight"))
        else:
            wqkv, bqkv = self._fz[f"{i}.wqkv"], self._fz[f"{i}.bqkv"]
            wo, w1, w2 = self._fz[f"{i}.wo"], self._fz[f"{i}.w1"], self._fz[f"{i}.w2"]
        return dict(wqkv=wqkv, bqkv=bqkv, wo=wo, bo=P_[pre + "self_attn.out_proj.bias"], w1=w1, b1=P_[pre + "mlp.fc1.bias"],
                    w2=w2, b2=P_[pre + "mlp.fc2.bias"], g1=P_[pre + "layer_norm1.weight"], be1=P_[pre + "layer_norm1.bias"],
                    g2=P_[pre + "layer_norm2.weight"], be2=P_[pre + "layer_norm2.bias"])

    # -- workspaces -----------------------------------------------------------------------------------
    def _touch_batch(self, B: int):
        """Workspaces are cached per batch size; only the `max_cached_batch_sizes` most recently used sizes are kept (a third size evicts the
        least recently used one's activations, saved layers and backward scratch -- the caching allocator reuses the memory).  A backward
        still pending for an evicted size finds a fresh workspace whose generation does not match and raises (autograd.OwlViTFunction)."""
        lru = self._ws_lru
        if lru and lru[0] == B:
            return
        if B in lru:
            lru.remove(B)
        lru.insert(0, B)
        # (with a deferred tail -- overlap_tail -- the backward / optimizer of the previous step may still be reading an evicted size's buffers
        #  on the tail stream, and the caching allocator hands freed memory to the NEXT allocation on the compute stream without waiting for
        #  other streams: order this stream behind the tail before anything is dropped)
        if len(lru) > max(1, int(self.max_cached_batch_sizes)) and self._tail_stream_ is not None:
            self._wait_params()
            torch.cuda.current_stream().wait_stream(self._tail_stream_)
        while len(lru) > max(1, int(self.max_cached_batch_sizes)):
            old = lru.pop()
            for k in [k for k in self._ws if (k if isinstance(k, int) else k[1]) == old]:
                del self._ws[k]

    def _patch_scratch(self, B):
        """im2row scratch of owl_patch_embed_bf16, sized by the library's own query (the dispatcher's rule lives in csrc/gemm.hip only): a patch size that is
        not 2^n on a problem too small for the ping-pong kernel needs one; L/14 at any batch size does not."""
        cfg = self.cfg
        nbytes = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_patch_embed_scratch_bytes_hw", B, *cfg.image_hw, cfg.patch_size, cfg.hidden, 0, nbytes)
        if int(nbytes.item()) == 0:
            return None
        key = ("im2row", B)
        if key not in self._ws:
            self._ws[key] = torch.zeros(int(nbytes.item()) // 2, dtype=torch.bfloat16, device=self.device_)
        return self._ws[key]

    @property
    def wide_head(self) -> bool:
        """More prompts than one 32-column MFMA tile holds (over 10 classes): the class head runs its wide kernels, forward and backward."""
        return self.cfg.queries > 32

    def _workspace(self, B: int, train: bool = True):
        """Activation workspace of batch size B.  Gradient-recording forwards and no-grad (eval) forwards use SEPARATE sets, so an
        eval forward between a training forward and its backward cannot overwrite what that backward reads; two recording forwards
        at the same batch size do share one set -- the autograd node checks `gen` and refuses to run on overwritten activations."""
        self._touch_batch(B)
        key = B if train else ("eval", B)
        if key in self._ws:
            return self._ws[key]
        cfg, dev = self.cfg, self.device_
        D, I, Tp, P, Dt, C = cfg.hidden, cfg.mlp, cfg.tokens_padded, cfg.patches, cfg.text_dim, cfg.n_classes
        M, Mh = B * Tp, B * P
        bf, f32 = torch.bfloat16, torch.float32
        z = ops.zeros_rows
        nqr = 32 * ops.wide_blocks(C) if self.wide_head else 32
        ws = dict(
            x=z(M, D, f32, dev), x_fin=z(M, D, f32, dev) if train else None, h=z(M, D, bf, dev), qkv=z(M, 3 * D, bf, dev),
            att=z(M, D, bf, dev), g=z(M, I, bf, dev), d1=z(M, D, bf, dev), d2=z(M, D, bf, dev),
            # heads
            cls_ln=torch.zeros(B, D, device=dev), feats=z(Mh, D, bf, dev), st_post=torch.zeros(M, 2, device=dev),
            st_pp=torch.zeros(Mh, 2, device=dev), hb0=z(Mh, D, bf, dev), ub0=z(Mh, D, bf, dev), hb1=z(Mh, D, bf, dev),
            ub1=z(Mh, D, bf, dev), sig=torch.zeros(Mh, 4, device=dev), e=z(Mh, Dt, f32, dev),
            # query table: [32, Dt] (<= 10 classes: one MFMA tile), or the wide head's [nblk][32][Dt] blocks of 10 classes (csrc/class_head_wide.hip)
            qhat=torch.zeros(nqr, Dt, device=dev), qnorm=torch.zeros(nqr, device=dev),
            argmax=torch.zeros(Mh, C, dtype=torch.uint8, device=dev), inv_norm=torch.zeros(Mh, device=dev),
            img=torch.zeros(B, 3, *cfg.image_hw, dtype=bf, device=dev),
            gen=0,          # set from the model-global counter by every recording forward (_forward_impl)
        )
        self._ws[key] = ws
        return ws

    def _layer_ws(self, B: int, i: int):
        """Saved activations of layer i (a layer the backward's dX chain crosses) for the backward; allocated once per batch size."""
        key = ("layer", B, i)
        if key in self._ws:
            return self._ws[key]
        cfg, dev = self.cfg, self.device_
        D, I, Tp = cfg.hidden, cfg.mlp, cfg.tokens_padded
        M = B * Tp
        bf, f32 = torch.bfloat16, torch.float32
        z = ops.zeros_rows
        L = dict(x_in=z(M, D, f32, dev), x_mid=z(M, D, f32, dev), st1=torch.zeros(M, 2, device=dev), st2=torch.zeros(M, 2, device=dev),
                 qkv=z(M, 3 * D, bf, dev), att=z(M, D, bf, dev),
                 lse=torch.zeros(B, cfg.heads, Tp, device=dev),
                 gp=z(M, I, bf, dev))          # quick_gelu'(u), saved by fc1's epilogue: what the dX GEMM through the activation multiplies by
        if i in self._tl_set:   # dW operands
            L.update(h1=z(M, D, bf, dev), h2=z(M, D, bf, dev), g=z(M, I, bf, dev))
        self._ws[key] = L
        return L

    def _pre_ws(self, B: int):
        """Kept by a gradient-recording forward when pre_layernorm or the embeddings train: the input of pre_layernorm and its row statistics; with trainable
        embeddings also the patch rows of the image (the patch-embedding weight gradient's X operand) and the packed bf16 gradient rows."""
        key = ("pre", B)
        if key in self._ws:
            return self._ws[key]
        cfg, dev = self.cfg, self.device_
        M, Mh = B * cfg.tokens_padded, B * cfg.patches
        L = dict(x_emb=ops.zeros_rows(M, cfg.hidden, torch.float32, dev), st_pre=torch.zeros(M, 2, device=dev))
        if self._train_emb:
            L.update(patches=ops.zeros_rows(Mh, (cfg.patch_k + 7) // 8 * 8, torch.bfloat16, dev), dE=ops.zeros_rows(Mh, cfg.hidden, torch.bfloat16, dev))
            if self._pos_used is not None:          # gradient of the resampled table [T, D], before the resampler's adjoint takes it to the native shape
                L["dU"] = torch.zeros(cfg.tokens, cfg.hidden, dtype=torch.float32, device=dev)
        self._ws[key] = L
        return L

    def _wt_specs(self):
        """(key, rows, cols) of every trainable weight the backward needs transposed (autograd.backward_impl): a parameter name, or `<layer prefix>qkv` for
        a layer's fused q / k / v weight."""
        cfg = self.cfg
        D, I, Dt = cfg.hidden, cfg.mlp, cfg.text_dim
        specs = [(n, r, c) for n, r, c in (("class_predictor.dense0.weight", Dt, D), ("box_head.dense1.weight", D, D), ("box_head.dense0.weight", D, D))
                 if n in self.flat_offsets and self.backward_floor != "heads"]
        for i in sorted(self.trainable_layers, reverse=True):
            tl = f"backbone.encoder.layers.{i}."
            specs += [(tl + "mlp.fc2.weight", D, I), (tl + "mlp.fc1.weight", I, D), (tl + "self_attn.out_proj.weight", D, D), (tl + "qkv", 3 * D, D)]
        return specs

    def _wqkv(self, i: int):
        """bf16 [3D, D] view of trainable layer i's fused q / k / v weight."""
        D = self.cfg.hidden
        o = self.flat_offsets[f"backbone.encoder.layers.{i}.self_attn.q_proj.weight"]
        return self.flat_bf16[o: o + 3 * D * D].view(3 * D, D)

    def _pretranspose_weights(self):
        """Launch the backward's weight transposes now, on their own stream (called by a gradient-recording forward on the stream that has just ordered itself
        behind any deferred optimizer step, right before the first trainable layer).  The backward waits for `_wt_event` and reads `_wt[key]`."""
        if self._wt is None:
            self._wt = {n: torch.empty(c, r, dtype=torch.bfloat16, device=self.device_) for n, r, c in self._wt_specs()}
            self._wt_stream_ = torch.cuda.Stream(device=self.device_)
        cur = torch.cuda.current_stream()
        s_ = self._wt_stream_
        s_.wait_stream(cur)                       # (the bf16 compute copies are current on `cur`; a previous backward's reads of these buffers precede this point on it too)
        with torch.cuda.stream(s_):
            for n, r, c in self._wt_specs():
                src = self._wqkv(int(n.split(".")[3])) if n.endswith(".qkv") else self._tview(n)
                ops.transpose_bf16(src, self._wt[n], r, c)
            ev = torch.cuda.Event()
            ev.record(s_)
        self._wt_event = ev

    def _refresh_patch_weight(self):
        """Trainable patch embedding with a patch size that is not 2^n: the forward's gather-layout weight follows the bucket's bf16 copy (every forward calls
        this right after that copy is known to be current, so it obeys the same staleness rule)."""
        if self._pe_gather is not None:
            dst, src = self._pe_gather
            w = self._tview("backbone.embeddings.patch_embedding.weight").view(self.cfg.hidden, self.cfg.patch_k)
            self._fz["w_pe"].index_copy_(1, dst, w.index_select(1, src))

    def _refresh_pos(self):
        """Run grid != native grid: the table the embeddings read follows the parameter (one launch; every forward with trainable embeddings calls it where
        the parameter is known to be current, i.e. behind _wait_params)."""
        self._invalidate_prefix()          # (a frozen table re-made: what the kept states were computed from may have changed)
        if self._pos_used is not None:
            cfg = self.cfg
            ops.pos_resample_hw(self._byname[_POS].detach(), self._pos_used, cfg.native_grid, cfg.grid_h, cfg.grid_w, cfg.hidden)

    def _pos_table(self):
        """The position table at the run grid: the parameter itself at the native size."""
        return self._byname[_POS] if self._pos_used is None else self._pos_used

    def refresh_compute_weights(self, force: bool = True):
        """bf16 copies of the trainable tensors: one cast over the flat bucket.  Every forward calls it, except the first forward after a
        fused AdamW step (whose kernel writes the copy itself and leaves a one-shot token, see __init__).  The only window left: a write
        that bypasses the version counter (`p.data.copy_()`, a raw-pointer kernel) BETWEEN FusedAdamW.step() and the next forward -- call
        this method after such a write.  force=True (a caller's own call, as opposed to a forward's) also empties the frozen-prefix activation cache:
        the caller is telling the model that tensors were written behind its back."""
        if force:
            self._invalidate_prefix()
        ops.cast_bf16(self.flat_param, self.flat_bf16)
        self._bf16_current = False
        self._refresh_patch_weight()

    def _mark_bf16_current(self):
        """optim.FusedAdamW.step only: its kernel has just rewritten flat_bf16 from the updated flat_param."""
        self._bf16_current = True
        self._bf16_version = self.flat_param._version

    def _apply(self, fn, recurse=True):
        """`.to()` / `.cuda()` / `.half()` / `.float()` / `.cpu()` replace every `param.data`, which would silently detach the 29 trainable
        tensors from the flat parameter / gradient / bf16 buckets the kernels read.  The model is built on its device in f32 (the reference's
        `.to(device)`, src/models.py:191, is done by construction): a call that changes nothing is accepted, anything else raises."""
        self._invalidate_prefix()
        probe = torch.empty(0, dtype=torch.float32, device=self.device_)
        out = fn(probe)
        if out.dtype != probe.dtype or out.device != probe.device:
            raise RuntimeError(
                f"OwlViT lives on {self.device_} in float32 (trainable tensors are views of one flat bucket; compute is bf16 inside the kernels): "
                f"moving / casting the module to {out.device} / {out.dtype} is not supported -- build it with load_model(labelmap, device)")
        return self

    # -- frozen-prefix activation cache ---------------------------------------------------------------------
    def enable_prefix_cache(self, max_bytes=None, max_images=None):
        """Switch the frozen-prefix activation cache on (prefix_cache.PrefixCache; max_bytes None = its DEFAULT_MAX_BYTES; slabs are allocated as they
        fill).  From then on `model(image, image_ids=ids)` keeps, per id, the f32 residual stream the first non-frozen consumer normalises -- the first
        LayerNorm of the lowest encoder layer the backward crosses, or the final LayerNorms under a heads-only set -- and skips the patch embedding,
        pre_layernorm and the encoder layers below it for ids already kept.  Same bits as without it.  An id must identify the PIXELS the model is
        handed: never pass ids together with a random augmentation.  Needs a frozen prefix: raises ValueError where layer 0, pre_layernorm or the
        embeddings train."""
        if self._chain_low == 0:
            keep = W.FREEZE_KEEP if self._keep is None else self._keep
            raise ValueError(f"enable_prefix_cache: the trainable set {tuple(keep)!r} leaves no frozen prefix (the backward reaches "
                             f"{self.backward_floor if not isinstance(self.backward_floor, int) else 'encoder layer 0'}): nothing below the first trainable tensor is constant")
        self.prefix_cache = PrefixCache(self.cfg.tokens_padded * self.cfg.hidden, max_bytes, max_images, self.device_, key=self.cfg)
        return self.prefix_cache

    def disable_prefix_cache(self):
        """Drop the cache and its slabs; `image_ids=` is refused again."""
        self.prefix_cache = None

    def _invalidate_prefix(self):
        if getattr(self, "prefix_cache", None) is not None:
            self.prefix_cache.clear()

    @staticmethod
    def _take_images(image, pos):
        """image[pos] for ascending positions, without an index tensor (which would be a host-to-device copy): the batch itself, or one concatenation of
        its runs."""
        if pos == list(range(image.shape[0])):
            return image
        runs, a = [], 0
        while a < len(pos):
            b = a
            while b + 1 < len(pos) and pos[b + 1] == pos[b] + 1:
                b += 1
            runs.append(image[pos[a]:pos[b] + 1])
            a = b + 1
        return runs[0] if len(runs) == 1 else torch.cat(runs)

    @property
    def _tail_stream(self):
        if self._tail_stream_ is None:
            self._tail_stream_ = torch.cuda.Stream(device=self.device_)
        return self._tail_stream_

    def finish(self):
        """Order the current stream behind a deferred tail (overlap_tail): call before reading parameters or gradients outside the model's own
        forward / backward / zero_grad / state_dict, which do it themselves."""
        self._wait_params()

    def _wait_params(self):
        """Order the compute stream behind a deferred optimizer step (ddp.DataParallel(overlap=True)): called right before the
        first trainable tensor is read, i.e. after the frozen prefix (under the reference rule: embeddings + encoder layers below the trainable one;
        with trainable embeddings or pre_layernorm there is no such prefix)."""
        if self._param_event is not None:
            torch.cuda.current_stream().wait_event(self._param_event)
            self._param_event = None

    def _check_trainable_set(self):
        """The backward is built at construction for one trainable set (`trainable=`; default: the reference's freeze rule, ref
        src/models.py:173-184).  The reference's rule is a user-editable loop over requires_grad; here a different set would silently
        get no gradient (or still be updated by the optimizer), so a mismatch is an error rather than a silent difference."""
        for n, p in self._byname.items():
            if p.requires_grad != (n in self._trainable):
                raise RuntimeError(
                    f"parameter `{n}` has requires_grad={p.requires_grad}, but this build's hand-written backward computes gradients for "
                    + ("exactly the reference's trainable set (layers.11 / box / post_layernorm / class_predictor / queries, ref "
                       "src/models.py:173-184)" if self._keep is None else
                       f"exactly the trainable set this model was built with (trainable={self._keep!r})")
                    + "; freezing or unfreezing individual tensors is not supported.  Choose the trainable set at construction: "
                    "load_model(..., trainable=[...]) / OwlViT(..., trainable=[...]).")

    # -- encoder schedule --------------------------------------------------------------------------------
    def _encoder_chunks(self, B: int):
        """[(first image, images)] of the sub-batches the encoder runs on separate streams.  Batches below 4 stay whole (train step, same process:
        batch 2 -7 %, batch 4 +8 %, batch 6 +0.5 %, batch 8 +4 % with two sub-batches)."""
        n = self.encoder_streams if B >= 4 else 1
        if n <= 1:
            return [(0, B)]
        base, extra = divmod(B, n)
        out, b0 = [], 0
        for c in range(n):
            nb = base + (1 if c < extra else 0)
            out.append((b0, nb)); b0 += nb
        return out

    @property
    def _dw_events(self):
        """Events of the backward's weight-gradient stream (autograd.backward_impl): four operand-ready events + the final join."""
        if self._dw_events_ is None:
            self._dw_events_ = [torch.cuda.Event() for _ in range(5)]
        return self._dw_events_

    def _side_stream(self, c: int):
        while len(self._streams) < c:
            self._streams.append(torch.cuda.Stream(device=self.device_))
            self._join[len(self._streams)] = torch.cuda.Event()
        return self._streams[c - 1]

    def _bwd_streams(self):
        """(side stream c, join event c, fork event) as the backward uses them: the forward's own in-line, a disjoint set as a deferred tail."""
        off = max(self.encoder_streams - 1, 1) if self.overlap_tail else 0
        if off and self._fork_ev_tail is None:
            self._fork_ev_tail = torch.cuda.Event()
        if not off and self._fork_ev is None:
            self._fork_ev = torch.cuda.Event()
        S = lambda c: self._side_stream(c + off)
        J = lambda c: (self._side_stream(c + off), self._join[c + off])[1]
        return S, J, (self._fork_ev_tail if off else self._fork_ev)

    def _encoder_layer(self, i: int, ws, B: int, save: bool, st):
        """Encoder layer i (HF5:478-511) for the sub-batch `st` (images [b0, b0 + nb) = rows [b0 Tp, (b0 + nb) Tp) of every buffer), on the
        current stream.  st carries the sub-batch's residual stream and the not-yet-added branch outputs from layer to layer."""
        cfg = self.cfg
        D, I, H, Tp, T = cfg.hidden, cfg.mlp, cfg.heads, cfg.tokens_padded, cfg.tokens
        b0, nb = st["b0"], st["nb"]
        r0, M = b0 * Tp, nb * Tp
        R = lambda t: t[r0:r0 + M]
        scale = cfg.head_dim ** -0.5
        xs, pending, pending1 = st["xs"], st["pending"], st["pending1"]
        d1, d2 = R(ws["d1"]), R(ws["d2"])
        lw = self._layer_weights(i)
        sv = save and self._chain_low is not None and i >= self._chain_low          # the backward passes through this layer: keep its activations
        full = sv and i in self._tl_set          # ... and, for a trainable layer, the dW operands too
        Ls = self._layer_ws(B, i) if sv else None
        st1 = R(Ls["st1"]) if sv else None
        h = R(Ls["h1"]) if full else R(ws["h"])
        # Residual adds (HF5:500,507) live in the LayerNorm kernels: the GEMM in front of each emits a bf16
        # delta through the fast wide-store epilogue, and LN does x += delta while it normalises.
        x_cur = R(Ls["x_in"]) if sv else xs
        if pending is None:
            if sv and x_cur.data_ptr() != xs.data_ptr():          # (the frozen-prefix cache hands the kept sum over in x_in itself)
                x_cur.copy_(xs)
            ops.layernorm(x_cur, lw["g1"], lw["be1"], h, M, D, st1, cfg.ln_eps)
        else:
            if pending1 is None:
                ops.layernorm(xs, lw["g1"], lw["be1"], h, M, D, st1, cfg.ln_eps, delta=pending, x_out=x_cur)
            else:       # (xs + delta1) + delta2, same operands and order as the two separate adds
                ops.layernorm(xs, lw["g1"], lw["be1"], h, M, D, st1, cfg.ln_eps, delta=pending1, delta2=pending, x_out=x_cur)
        # ONE row-major QKV GEMM per layer.  The attention kernels (forward and backward) read every transposed MFMA operand
        # (V^T; Q^T, K^T, dO^T) out of the row-major tiles with the LDS hardware transpose (ds_read_b64_tr_b16): no transposed
        # copy of anything exists in HBM.
        qkv_l = R(Ls["qkv"]) if sv else R(ws["qkv"])
        cc = st.get("conc", 1)          # sub-batch streams in flight: small problems running ALONE take half-height GEMM tiles (ops.gemm)
        ops.gemm(ops.EPI_BIAS_BF16, h, lw["wqkv"], qkv_l, bias=lw["bqkv"], M=M, N=3 * D, K=D, ldo=3 * D, concurrency=cc)
        att_l = R(Ls["att"]) if sv else R(ws["att"])
        ops.attention_fwd_vrow(qkv_l, qkv_l[:, D:], qkv_l[:, 2 * D:], 3 * D, att_l, D, Ls["lse"][b0:b0 + nb] if sv else None, nb, H, T, Tp, scale)
        ops.gemm(ops.EPI_BIAS_BF16, att_l, lw["wo"], d1, bias=lw["bo"], M=M, N=D, K=D, concurrency=cc)
        x_mid = R(Ls["x_mid"]) if sv else x_cur
        h2 = R(Ls["h2"]) if full else R(ws["h"])
        # A frozen layer's x + delta1 is read by nobody but the next LayerNorm: it is not stored (4 bytes per element), that
        # LayerNorm adds both branch outputs instead (2 more bytes read).  Layers whose activations are kept, and the last one
        # (the merge kernel takes a single delta), store it.
        defer = (not sv) and (i + 1 < cfg.layers)
        ops.layernorm(x_cur, lw["g2"], lw["be2"], h2, M, D, R(Ls["st2"]) if sv else None, cfg.ln_eps, delta=d1, x_out=x_mid,
                      store_x=not defer)
        g_l = R(Ls["g"]) if full else R(ws["g"])
        ops.gemm(ops.EPI_QGELU_BF16, h2, lw["w1"], g_l, bias=lw["b1"], aux=R(Ls["gp"]) if sv else None, M=M, N=I, K=D, concurrency=cc)
        ops.gemm(ops.EPI_BIAS_BF16, g_l, lw["w2"], d2, bias=lw["b2"], M=M, N=D, K=I, concurrency=cc)
        st["pending"], st["xs"] = d2, x_mid
        st["pending1"] = d1 if defer else None

    # -- forward ---------------------------------------------------------------------------------------
    def _forward_impl(self, image: torch.Tensor, save: bool, ids=None):
        """ids (list of B ints, forward() has checked them; None = no cache): the frozen-prefix cache's path -- the input stage and the encoder layers below
        the boundary run on the images not yet kept, compacted to the first rows of the same workspace, then the kept and the fresh states meet in the
        boundary buffer and the rest runs on the whole batch as ever."""
        cfg = self.cfg
        D, I, H, Tp, T, P, Dt, C = cfg.hidden, cfg.mlp, cfg.heads, cfg.tokens_padded, cfg.tokens, cfg.patches, cfg.text_dim, cfg.n_classes
        B = image.shape[0] if ids is None else len(ids)
        if image is not None and tuple(image.shape[1:]) != (3, *cfg.image_hw):
            raise ValueError(f"image must be [B,3,{cfg.image_hw[0]},{cfg.image_hw[1]}], got {tuple(image.shape)}")
        plan = None
        if ids is not None:
            cache = self.prefix_cache
            if cache.key != cfg:          # kept states belong to one size and architecture
                cache.clear()
                cache.key = cfg
            plan = cache.plan(ids)
            if image is None and plan.miss_ids:
                raise ValueError(f"image=None needs every id in the prefix cache; not kept: {plan.miss_ids}")
        Bp = B if plan is None else len(plan.miss_pos)          # images the input stage and the frozen prefix run on
        ws = self._workspace(B, train=save)
        # model-global, monotonically increasing: a workspace rebuilt after an LRU eviction can never carry a generation an older autograd
        # node still holds (a per-workspace counter restarted at 0 and could collide: fwd(A) -> two other sizes evict A -> fwd(A) again)
        self._gen += 1
        ws["gen"] = self._gen
        M, Mh = B * Tp, B * P
        P_ = self._byname
        if self._bf16_current and self._bf16_version == self.flat_param._version:
            self._bf16_current = False          # one-shot: the fused AdamW's own bf16 pass covers exactly this forward
            from_optimizer = True
        else:
            from_optimizer = False
            self._wait_params()
            self.refresh_compute_weights(force=False)
        if self._train_emb or self._train_pre:
            # the first trainable tensor is read by the embeddings (and a deferred tail's backward may still be reading the kept bf16 image): nothing of this
            # forward runs under a deferred tail
            self._wait_params()
            if from_optimizer:
                self._refresh_patch_weight()        # (the other branch above has done it: refresh_compute_weights)
            if self._train_emb:
                self._refresh_pos()                 # behind the wait above: the deferred tail's AdamW has written the table this reads

        if plan is not None and 0 < Bp < B:
            image = self._take_images(image, plan.miss_pos)
        if Bp == 0:
            img = None          # every image's boundary state is kept: none of the input stage runs
        elif image.dtype == torch.float32:
            ops.cast_bf16(image.contiguous(), ws["img"])
            img = ws["img"]
        elif image.dtype == torch.bfloat16:
            img = image.contiguous()
        else:
            raise TypeError("image must be float32 or bfloat16")

        x = ws["x"]
        pos = self._pos_table()
        low = save and self.backward_floor in ("pre_layernorm", "embeddings")
        if Bp == 0:
            pass
        elif low:
            # the backward goes below layer 0: keep pre_layernorm's input and row statistics (and, for the patch-embedding weight gradient, the bf16 image)
            pw = self._pre_ws(B)
            if self._train_emb and img is not ws["img"]:
                ws["img"].copy_(img)
            x_emb = pw["x_emb"]
            ops.patch_embed_hw(img, self._fz["w_pe"], pos, x_emb, B, *cfg.image_hw,
                               cfg.patch_size, D, Tp, scratch=self._patch_scratch(B))
            ops.cls_rows(x_emb, P_["backbone.embeddings.class_embedding"], pos, B, Tp, D)
            ops.layernorm(x_emb, P_["backbone.pre_layernorm.weight"], P_["backbone.pre_layernorm.bias"], x, M, D, pw["st_pre"], cfg.ln_eps)
        else:
            ops.patch_embed_hw(img, self._fz["w_pe"], pos, x, Bp, *cfg.image_hw,
                               cfg.patch_size, D, Tp, scratch=self._patch_scratch(Bp))
            ops.cls_rows(x, P_["backbone.embeddings.class_embedding"], pos, Bp, Tp, D)
            ops.layernorm(x, P_["backbone.pre_layernorm.weight"], P_["backbone.pre_layernorm.bias"], x, Bp * Tp, D, eps=cfg.ln_eps)

        # ---- encoder.  No kernel of it couples images, so the batch is run as `encoder_streams` sub-batches (contiguous row ranges of the
        #      same buffers), each on its own HIP stream, layer by layer: the idle CUs of one sub-batch's last GEMM round / attention tail
        #      run the other sub-batch's next kernel (a 256 x 256 GEMM workgroup owns its CU's registers and LDS, so the overlap is at CU
        #      granularity).  Measured on the forward: -3.7 % at B/16 batch 32, -2.9 % at L/14 batch 16 (two streams; three or four lose --
        #      profiles/r02_encoder_streams.md).  Every kernel is batch-invariant: same bits as the single-stream schedule.
        # first encoder layer that reads a trainable tensor (or keeps an activation the deferred tail's backward may still be reading): where the sub-batch
        # streams wait for a deferred tail.  None: no encoder layer does; the wait then sits in front of the final LayerNorms.
        tl = self._chain_low
        param_event, self._param_event = self._param_event, None
        main = torch.cuda.current_stream()
        if save and tl is not None:        # first use allocates (and zero-fills, on THIS stream) the kept activations: before any other stream may write them
            for i in range(tl, cfg.layers):
                self._layer_ws(B, i)

        def run_layers(lo, hi, nb_all, buf):
            """Layers [lo, hi) on images [0, nb_all), whose residual stream enters in `buf`, as sub-batches on their streams; joined on `main`."""
            nonlocal param_event
            chunks = self._encoder_chunks(nb_all)
            if len(chunks) > 1:
                if self._fork_ev is None:
                    self._fork_ev = torch.cuda.Event()
                self._fork_ev.record(main)
            states = []
            for c, (b0, nb) in enumerate(chunks):
                st = dict(b0=b0, nb=nb, stream=main if c == 0 else self._side_stream(c), xs=buf[b0 * Tp:(b0 + nb) * Tp], pending=None, pending1=None, conc=len(chunks))
                if c > 0:
                    st["stream"].wait_event(self._fork_ev)
                states.append(st)
            for i in range(lo, hi):
                for st in states:
                    with torch.cuda.stream(st["stream"]):
                        if i == tl and param_event is not None:
                            st["stream"].wait_event(param_event)    # everything above ran on frozen weights only (ddp overlap schedule)
                        if i == tl and save and self.pretranspose and st is states[0]:
                            self._pretranspose_weights()            # the backward's W^T copies, beside the rest of this forward and the loss chain
                        self._encoder_layer(i, ws, B, save, st)
            for c, st in enumerate(states):
                if c > 0:
                    self._join[c].record(st["stream"])
                    main.wait_event(self._join[c])
            return states

        last = cfg.layers - 1
        chunks = self._encoder_chunks(B)          # (the whole batch's: what the heads' fork below goes by)
        if plan is None:
            states = run_layers(0, cfg.layers, B, x)
            # the sub-batches' residual streams / deferred MLP-branch outputs are row ranges of ONE buffer each: the merge kernel takes the batch
            if tl is None and param_event is not None:
                main.wait_event(param_event)            # heads-only sets: the whole encoder ran on frozen weights
            xs = self._layer_ws(B, last)["x_mid"] if (save and tl is not None) else x
            pending = ws["d2"]
        else:
            # ---- frozen-prefix cache: layers below the boundary on the compacted misses (rows [0, Bp Tp) of the same buffers); then, on the main stream, the
            #      fresh sums go to their positions and slots and the kept ones are copied in; layers from the boundary up on the whole batch.  The boundary
            #      buffer is what the first non-frozen consumer reads anyway where the backward keeps it (x_in of layer tl; x_fin under a heads-only set) and
            #      a buffer of the workspace's own otherwise -- never `x`, which holds the compacted source.
            first = cfg.layers if tl is None else tl
            pre = run_layers(0, first, Bp, x) if Bp else []
            if param_event is not None:
                # the boundary buffer and everything above are what a deferred tail's backward may still be reading; the streams of the second leg fork
                # from this one behind the wait
                main.wait_event(param_event)
                param_event = None
            if save:
                bound = self._layer_ws(B, tl)["x_in"] if tl is not None else ws["x_fin"]
            else:
                if "x_pc" not in ws:
                    ws["x_pc"] = ops.zeros_rows(M, D, torch.float32, self.device_)
                bound = ws["x_pc"]
            if pre:
                assert all(st["xs"].data_ptr() == x.data_ptr() + st["b0"] * Tp * D * 4 and st["pending"] is not None for st in pre)
                d1 = ws["d1"] if pre[0]["pending1"] is not None else None          # (xs + d1) + d2: the operands and order of the LayerNorm that would have read them
                deltas = (d1, ws["d2"]) if d1 is not None else (ws["d2"], None)
                cache.fill(plan, bound, x, *deltas)
            else:
                cache.fill(plan, bound)
            states = run_layers(first, cfg.layers, B, bound)
            if tl is None:
                xs, pending = bound, None          # the kept sum IS the final residual stream: the merge kernel's no-delta form (the backward reads it where it lies)
            else:
                xs, pending = (self._layer_ws(B, last)["x_mid"] if save else bound), ws["d2"]
        assert all(st["xs"].data_ptr() == xs.data_ptr() + st["b0"] * Tp * D * 4 for st in states)

        # ---- final residual add + post_layernorm (all tokens) * class token -> post_post_layernorm
        #      (ref src/models.py:80-86); the final residual stream is materialised in `x` for the backward
        feats = ws["feats"]
        tv = self._hw
        # (the backward reads the final residual stream; it gets a buffer of its own because with overlap_tail the NEXT forward's patch embedding
        #  rewrites `x` while this step's backward may still be running)
        ops.merge_ln(xs, P_["backbone.post_layernorm.weight"], P_["backbone.post_layernorm.bias"], P_["post_post_layernorm.weight"],
                     P_["post_post_layernorm.bias"], ws["cls_ln"], feats, ws["st_post"], ws["st_pp"], B, P, Tp, D, cfg.ln_eps,
                     delta=pending, x_out=ws["x_fin"] if save else x)
        # The box head and the class head only share their input: with sub-batch streams on, the class head runs on the side stream beside the
        # box head (its kernels fill the CUs the box GEMMs' remainder rounds leave idle).  Outputs are allocated before the fork.
        pred_boxes = torch.empty(B, P, 4, device=self.device_)
        pred_sims = torch.empty(B, P, C, device=self.device_)
        side = self._side_stream(1) if (self.head_streams and self.encoder_streams > 1 and len(chunks) > 1) else None
        if side is not None:
            self._fork_ev.record(main)
            side.wait_event(self._fork_ev)
        # ---- class head (ref src/models.py:24-38) ------------------------------------------------------
        with torch.cuda.stream(side if side is not None else main):
            ops.gemm(ops.EPI_F32, feats, tv("class_predictor.dense0.weight"), ws["e"], bias=P_["class_predictor.dense0.bias"], M=Mh, N=Dt, K=D)
            if self.wide_head:          # label sets beyond 10 classes: the query blocks of csrc/class_head_wide.hip
                ops.query_normalize_wide(P_["queries"], ws["qhat"], ws["qnorm"], cfg.queries, Dt)
                ops.class_sims_wide(ws["e"], ws["qhat"], pred_sims, ws["argmax"], ws["inv_norm"], Mh, Dt, C)
            else:
                ops.query_normalize(P_["queries"], ws["qhat"], ws["qnorm"], cfg.queries, Dt)
                ops.class_sims(ws["e"], ws["qhat"], pred_sims, ws["argmax"], ws["inv_norm"], Mh, Dt, C)
        # ---- box head (HF5:983-999) + bias / sigmoid / corners ---------------------------------------
        ops.gemm(ops.EPI_GELU_BF16, feats, tv("box_head.dense0.weight"), ws["hb0"], bias=P_["box_head.dense0.bias"],
                 aux=ws["ub0"] if save else None, M=Mh, N=D, K=D)
        ops.gemm(ops.EPI_GELU_BF16, ws["hb0"], tv("box_head.dense1.weight"), ws["hb1"], bias=P_["box_head.dense1.bias"],
                 aux=ws["ub1"] if save else None, M=Mh, N=D, K=D)
        ops.box_final(ws["hb1"], P_["box_head.dense2.weight"], P_["box_head.dense2.bias"], self.box_bias, pred_boxes, ws["sig"], Mh, P, D)
        if side is not None:
            self._join[1].record(side)
            main.wait_event(self._join[1])
        return pred_boxes, pred_sims

    def forward(self, image: torch.Tensor, image_ids=None):
        """ref src/models.py:98-119: returns (pred_boxes xyxy, None, pred_sims, None).

        image_ids (None = no cache, today's path): B integers (a sequence or a CPU tensor; a device tensor is refused: reading it would be a sync) that
        identify the pixels of each image, e.g. the dataset index -- see enable_prefix_cache().  `image` may be None when every id is kept."""
        ids = None
        if image_ids is not None:
            if self.prefix_cache is None:
                raise RuntimeError("image_ids= needs the frozen-prefix cache: call model.enable_prefix_cache() first")
            ids = _id_list(image_ids)
            if image is not None and image.shape[0] != len(ids):
                raise ValueError(f"image_ids has {len(ids)} entries for a batch of {image.shape[0]} images")
            if not ids:
                raise ValueError("image_ids is empty")
        elif image is None:
            raise ValueError("image=None needs image_ids= (and every id kept by the prefix cache)")
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if need_grad:
            self._check_trainable_set()
            from .autograd import OwlViTFunction
            names = list(self.flat_offsets.keys())
            boxes, sims = OwlViTFunction.apply(self, image, ids, *[self._byname[n] for n in names])
        else:
            boxes, sims = self._forward_impl(image, save=False, ids=ids)
        return (boxes, None, sims, None)

    # -- query bank from image exemplars ---------------------------------------------------------------------
    def _embed_image_query(self, pixel_values, query_boxes):
        cfg, dev = self.cfg, self.device_
        P, Dt = cfg.patches, cfg.text_dim
        N = int(pixel_values.shape[0])
        if N < 1:
            raise ValueError("embed_image_query: no images")
        qb = None
        if query_boxes is not None:
            qb = torch.as_tensor(query_boxes, dtype=torch.float32).to(dev).contiguous()
            if tuple(qb.shape) != (N, 4):
                raise ValueError(f"embed_image_query: query_boxes must be [{N}, 4] normalised corners (x0, y0, x1, y1), got {tuple(qb.shape)}")
        self._wait_params()
        queries, best, boxes, info = [], [], [], []
        # at most two batch sizes are new to the workspace cache (full chunks and the last one): with the limit raised by two for the length of this call
        # no size is evicted by it, so a recording forward's pending backward still finds its activations
        keep = self.max_cached_batch_sizes
        self.max_cached_batch_sizes = max(1, int(keep)) + 2
        try:
            for a in range(0, N, EXEMPLAR_CHUNK):
                nb = min(EXEMPLAR_CHUNK, N - a)
                pb, _ = self._forward_impl(pixel_values[a:a + nb], save=False)
                e = self._workspace(nb, train=False)["e"]          # the class head's dense0 output of this chunk: read before the next chunk overwrites it
                b, q, i = ops.image_query_select(e, pb, None if qb is None else qb[a:a + nb], nb, P, Dt)
                queries.append(q); best.append(b); boxes.append(pb); info.append(i)
        finally:
            self.max_cached_batch_sizes = keep
        cat = (lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts))
        return cat(queries), cat(best).to(torch.int64), cat(boxes), cat(info)

    @torch.no_grad()
    def embed_image_query(self, pixel_values, query_boxes=None):
        """OWL-ViT's image-conditioned query (HF `OwlViTForObjectDetection.embed_image_query`, same names and return order): for each example image, among
        the predicted boxes whose IoU with the query box is within 80 % of the best, the one whose class embedding is least like the image's mean
        embedding; its un-normalised class embedding is the query.  -> (query_embeds [N, Dt] f32, box_indices [N] int64, pred_boxes [N, P, 4]).

        query_boxes: [N, 4] normalised corners (x0, y0, x1, y1) of the annotated object inside each processed image, on any device; None = the whole
        image, which is the rule HF hard-wires.  HF's quirks are kept (csrc/image_query.hip): when no box overlaps, the generalized IoU decides and only
        an exactly touching box can be selected; an image HF would silently drop is reported with index -1 and a zero embedding.

        Runs without grad on the EVAL workspace (a pending training backward is not disturbed), behind a deferred optimizer tail, in chunks of at
        most 32 images; no host sync.  The frozen-prefix cache is neither read nor written."""
        return self._embed_image_query(pixel_values, query_boxes)[:3]

    @torch.no_grad()
    def set_queries_from_exemplars(self, pixel_values, class_ids, query_boxes=None):
        """Initialise the query bank from annotated example images: exemplar n (pixel_values[n], optionally its object's box query_boxes[n]) belongs to
        class class_ids[n].  The exemplars of a class are numbered k = 0, 1, ... in the order given; slot s in {0, 1, 2} of class c (bank row 3 c + s)
        becomes the unit mean of the unit queries {k : k % 3 == s}, or, when that set is empty, of exemplar s % n_c (exemplar_slots).  A class without
        exemplars keeps its three rows, bit for bit -- a text prior stays where no image prior is given.

        Writes the `queries` parameter in place (one kernel, on its flat-bucket view).  Reading the selection back is ONE host sync: this is
        initialisation and never runs inside a step.  Call it BEFORE constructing FusedAdamW / ddp.DataParallel: Adam moments and an EMA are not
        rewritten (under data parallel every rank computes the same bits from the same exemplars, or the wrapper broadcasts rank 0's bank as it does
        today).  The frozen-prefix cache stays valid: the bank sits above it.

        Raises ValueError naming the exemplar and its class when a class id is outside [0, C), a box is not x0 < x1, y0 < y1, or a selection is empty
        (no predicted box overlaps or touches the query box); RuntimeError inside `optimizer.ema_weights()`.
        -> dict(box_indices [N], n_selected [N], fallback [N] (lists of int / bool), slots = the 3 C member lists)."""
        if getattr(self, "_ema_scope", False):
            raise RuntimeError("set_queries_from_exemplars inside `with ema_weights():` -- the bucket holds the averaged weights and the raw iterate is stashed: "
                               "leave the scope first")
        cfg = self.cfg
        ids = check_exemplars(class_ids, query_boxes, int(pixel_values.shape[0]), cfg.n_classes)
        table = exemplar_slots(ids, cfg.n_classes)
        query, best, _, info = self._embed_image_query(pixel_values, query_boxes)
        host = torch.cat([best.view(-1, 1).to(torch.int32), info], 1).cpu().tolist()          # the one sync
        for n, (b, flags, nsel) in enumerate(host):
            if b < 0 or flags & 2:
                raise ValueError(f"set_queries_from_exemplars: exemplar {n} (class {ids[n]}) selects no predicted box: none overlaps or exactly touches its "
                                 "query box")
        row_ptr, members = slots_csr(table)
        dev = self.device_
        bank = self._byname["queries"].data.view(cfg.queries, cfg.text_dim)
        ops.query_bank_fill(query, torch.from_numpy(row_ptr).to(dev), torch.from_numpy(members).to(dev), bank, len(ids), cfg.queries, cfg.text_dim)
        self._bf16_current = False          # a raw-pointer write the bucket's version counter does not see: the next forward recasts the bf16 copy
        return dict(box_indices=[h[0] for h in host], n_selected=[h[2] for h in host], fallback=[bool(h[1] & 1) for h in host], slots=table)

    # -- zero-shot inference: HF's class head over per-image text / image queries ---------------------------------------------
    def set_logit_head(self, head, trainable=False):
        """head: weights.hf_logit_head(sd) -- {"logit_shift.weight" [D], "logit_shift.bias" [], "logit_scale.weight" [D], "logit_scale.bias" []} (arrays
        or tensors).  They become frozen f32 device buffers in `model.logit_head`, outside flat_param, parameters() and state_dict(): nothing trains
        through them and no checkpoint changes.  None removes them.  ValueError names a tensor of the wrong size, KeyError a missing one.

        trainable=True: the four tensors live in ONE flat f32 device buffer of 2 D + 2 elements, laid out w_shift | w_scale | b_shift | b_scale, and
        `model.logit_head` holds four leaf views of it with requires_grad=True (the same four keys: detect, forward_queries and the backward read the
        same storage).  `forward_queries`' backward then gives them ordinary autograd gradients (csrc/open_vocab_bwd.hip, owl_class_logits_bwd_head).
        They are still NOT registered parameters: parameters(), named_parameters(), state_dict(), flat_param / flat_grad / flat_offsets, FusedAdamW, its
        EMA and ddp.DataParallel see nothing new, and no `trainable=` substring reaches them.  The caller steps them with a torch optimizer over
        `model.logit_head_parameters()` -- the contract of a learnable `query_embeds` -- and writes them back to HF through `model.logit_head_state()`."""
        if head is None:
            self.logit_head = None
            self._logit_head_flat = None
            return self
        D, out = self.cfg.hidden, {}
        for k in W.LOGIT_HEAD_KEYS:
            if k not in head:
                raise KeyError(f"set_logit_head: `{k}` is missing (weights.hf_logit_head builds the four tensors)")
            t = torch.as_tensor(np.asarray(head[k].detach().cpu() if torch.is_tensor(head[k]) else head[k]), dtype=torch.float32).reshape(-1)
            want = D if k.endswith("weight") else 1
            if t.numel() != want:
                raise ValueError(f"set_logit_head: `{k}` must have {want} element(s) for hidden size {D}, got {t.numel()}")
            out[k] = t.contiguous().to(self.device_)
        if trainable:
            flat = torch.cat([out["logit_shift.weight"], out["logit_scale.weight"], out["logit_shift.bias"], out["logit_scale.bias"]])
            at = {"logit_shift.weight": (0, D), "logit_scale.weight": (D, 2 * D), "logit_shift.bias": (2 * D, 2 * D + 1), "logit_scale.bias": (2 * D + 1, 2 * D + 2)}
            out = {k: flat[at[k][0]:at[k][1]].detach().requires_grad_(True) for k in W.LOGIT_HEAD_KEYS}          # leaves that share the buffer's storage
            self._logit_head_flat = flat
        else:
            self._logit_head_flat = None
        self.logit_head = out
        return self

    def logit_head_parameters(self):
        """The four leaf tensors of a trainable logit head (set_logit_head(head, trainable=True)), in weights.LOGIT_HEAD_KEYS' order, for a torch
        optimizer of the caller's.  A frozen head, or none, gives an EMPTY list: torch.optim refuses it ("optimizer got an empty parameter list"), and
        `params + model.logit_head_parameters()` adds nothing."""
        lh = getattr(self, "logit_head", None)
        if lh is None:
            return []
        return [lh[k] for k in W.LOGIT_HEAD_KEYS if lh[k].requires_grad]

    def logit_head_state(self):
        """The logit head as weights.hf_logit_head gives it -- float32 numpy, HF's shapes ([D] weights, 0-d biases) -- trained or not: prefix the keys
        with `class_head.` (HF's weights are [1, D], biases [1]) to put a trained head back into an `OwlViTForObjectDetection` state dict;
        `set_logit_head(model.logit_head_state())` restores the same bits.  A host copy (it synchronises)."""
        lh = getattr(self, "logit_head", None)
        if lh is None:
            raise RuntimeError("logit_head_state: no logit head -- call model.set_logit_head(weights.hf_logit_head(hf_state_dict)) or load_model(..., logit_head=)")
        out = OrderedDict()
        for k in W.LOGIT_HEAD_KEYS:
            v = lh[k].detach().cpu().numpy().astype(np.float32)
            out[k] = np.ascontiguousarray(v.reshape(-1)) if k.endswith("weight") else v.reshape(()).copy()
        return out

    # -- OWLv2's objectness head: HF's `objectness_predictor` on the detached image features -------------------------------------
    def _objectness_layout(self):
        """Where the six tensors sit in the head's flat f32 buffer (parameters and gradient alike): dense0.weight | dense0.bias | dense1.weight | dense1.bias |
        dense2.weight | dense2.bias | three pad zeros (the tail's reducer writes dw2, db2 in quads) -> ({key: (begin, end, shape)}, elements)."""
        D = self.cfg.hidden
        at, o = {}, 0
        for k, shape in zip(W.OBJECTNESS_HEAD_KEYS, ((D, D), (D,), (D, D), (D,), (D,), (1,))):
            n = int(np.prod(shape))
            at[k] = (o, o + n, shape)
            o += n
        return at, o + 3

    def set_objectness_head(self, head, trainable=False):
        """head: weights.hf_objectness_head(sd) -- {"dense0.weight" [D, D], "dense0.bias" [D], "dense1.weight" [D, D], "dense1.bias" [D], "dense2.weight" [D],
        "dense2.bias" []} (arrays or tensors; HF's [1, D] / [1] shapes of dense2 are taken too).  They become frozen f32 device buffers in
        `model.objectness_head` plus bf16 copies of the two D x D weights for the GEMMs, outside flat_param, parameters() and state_dict().  None removes
        them.  ValueError names a tensor of the wrong size, KeyError a missing one.

        trainable=True: the six tensors live in ONE flat f32 device buffer (_objectness_layout) and `model.objectness_head` holds six leaf views of it with
        requires_grad=True; the bf16 copies are re-cast behind every forward that reads them.  `forward_queries(..., objectness=True)` then gives them
        ordinary autograd gradients (autograd.OwlViTObjectnessFunction).  They are still NOT registered parameters: parameters(), state_dict(), flat_param /
        flat_grad, FusedAdamW, its EMA and ddp.DataParallel see nothing new, and no `trainable=` substring reaches them.  The caller steps them with a torch
        optimizer over `model.objectness_head_parameters()` (and all-reduces their gradients under data parallel) and writes them back to HF through
        `model.objectness_head_state()`.  The head reads the features DETACHED, as HF does: no gradient of it reaches the trunk."""
        if head is None:
            self.objectness_head = self._objectness_flat = self._objectness_bf16 = None
            return self
        at, n = self._objectness_layout()
        flat = torch.zeros(n, dtype=torch.float32)
        for k in W.OBJECTNESS_HEAD_KEYS:
            if k not in head:
                raise KeyError(f"set_objectness_head: `{k}` is missing (weights.hf_objectness_head builds the six tensors)")
            t = torch.as_tensor(np.asarray(head[k].detach().cpu() if torch.is_tensor(head[k]) else head[k]), dtype=torch.float32)
            a, b, shape = at[k]
            ok = t.numel() == b - a and (tuple(t.shape) == shape or k.startswith("dense2"))
            if not ok:
                raise ValueError(f"set_objectness_head: `{k}` must be {list(shape)} for hidden size {self.cfg.hidden}, got {list(t.shape)}")
            flat[a:b] = t.reshape(-1)
        flat = flat.to(self.device_)
        views = {k: flat[at[k][0]:at[k][1]].view(at[k][2]) for k in W.OBJECTNESS_HEAD_KEYS}
        if trainable:
            views = {k: v.detach().requires_grad_(True) for k, v in views.items()}          # leaves that share the buffer's storage
        self._objectness_flat = flat if trainable else None
        self.objectness_head = views
        self._objectness_bf16 = {k: ops.cast_bf16(views[k].detach()) for k in ("dense0.weight", "dense1.weight")}
        return self

    def objectness_head_parameters(self):
        """The six leaf tensors of a trainable objectness head, in weights.OBJECTNESS_HEAD_KEYS' order, for a torch optimizer of the caller's.  A frozen
        head, or none, gives an EMPTY list."""
        oh = getattr(self, "objectness_head", None)
        if oh is None:
            return []
        return [oh[k] for k in W.OBJECTNESS_HEAD_KEYS if oh[k].requires_grad]

    def objectness_head_state(self):
        """The objectness head in HF's shapes -- float32 numpy, dense0 / dense1 [D, D] and [D], dense2.weight [1, D], dense2.bias [1] -- trained or not: prefix
        the keys with `objectness_head.` and the six tensors go straight back into an `Owlv2ForObjectDetection` state dict (`load_state_dict` takes them).
        `set_objectness_head(model.objectness_head_state())` restores the same bits (it takes HF's shapes and weights.hf_objectness_head's alike).  A host
        copy (it synchronises)."""
        oh = getattr(self, "objectness_head", None)
        if oh is None:
            raise RuntimeError("objectness_head_state: no objectness head -- call model.set_objectness_head(weights.hf_objectness_head(hf_state_dict)) "
                               "or load_model(..., objectness_head=)")
        out = OrderedDict()
        for k in W.OBJECTNESS_HEAD_KEYS:
            v = oh[k].detach().cpu().numpy().astype(np.float32)
            out[k] = np.ascontiguousarray(v.reshape(1, -1) if k == "dense2.weight" else v)          # (dense2.bias is held as [1]: HF's shape)
        return out

    def _need_objectness(self, who):
        if self.objectness_head is None:
            raise RuntimeError(f"{who}: no objectness head -- call model.set_objectness_head(weights.hf_objectness_head(hf_state_dict)) or "
                               "load_model(..., objectness_head=)")

    def _objectness_on(self, feats, h0, h1, out, rows, u0=None, u1=None):
        """The head on `rows` rows of bf16 features: two erf-GELU GEMMs into h0 / h1 (pre-activations kept in u0 / u1 when given) and the row-dot tail ->
        out (f32, `rows` elements).  Three launches, one more pair where a trainable head's bf16 weights are re-cast."""
        oh, wb, D = self.objectness_head, self._objectness_bf16, self.cfg.hidden
        if self._objectness_flat is not None:
            for k in wb:
                ops.cast_bf16(oh[k].detach(), wb[k])
        ops.gemm(ops.EPI_GELU_BF16, feats, wb["dense0.weight"], h0, bias=oh["dense0.bias"].detach(), aux=u0, M=rows, N=D, K=D)
        ops.gemm(ops.EPI_GELU_BF16, h0, wb["dense1.weight"], h1, bias=oh["dense1.bias"].detach(), aux=u1, M=rows, N=D, K=D)
        return ops.objectness_final(h1, oh["dense2.weight"].detach(), oh["dense2.bias"].detach(), out, rows, D)

    def _objectness_ws(self, B):
        """The head's own activations on the TRAINING path, allocated when first needed at this batch size: h0, u0, h1, u1 bf16 [B P, D] (hb0 / ub0 / hb1 /
        ub1 belong to the box head's backward)."""
        key = ("obj", B)
        if key not in self._ws:
            Mh, D, z = B * self.cfg.patches, self.cfg.hidden, ops.zeros_rows
            self._ws[key] = {k: z(Mh, D, torch.bfloat16, self.device_) for k in ("h0", "u0", "h1", "u1")}
        return self._ws[key]

    def _objectness_train_forward(self, B):
        """The head on the training workspace's feats (the recording forward of this batch size has just run) -> objectness_logits f32 [B, P]."""
        ws, ow, P = self._workspace(B), self._objectness_ws(B), self.cfg.patches
        out = torch.empty(B, P, dtype=torch.float32, device=self.device_)
        self._objectness_on(ws["feats"], ow["h0"], ow["h1"], out, B * P, u0=ow["u0"], u1=ow["u1"])
        return out

    @torch.no_grad()
    def detect(self, pixel_values, query_embeds, query_mask=None, return_scores=False, objectness=False):
        """Zero-shot detection, HF `OwlViTForObjectDetection` logits: -> (pred_boxes [B, P, 4], logits [B, P, Q]) and, with return_scores=True,
        scores = sigmoid(logits) [B, P, Q] (exactly 0 where masked).  pred_boxes are CORNERS (x0, y0, x1, y1), as everywhere in this project; HF's
        `pred_boxes` are (cx, cy, w, h).

        query_embeds: f32 [B, Q, Dt] (a bank per image) or [Q, Dt] (one bank shared by the batch, read where it lies: no copy per image), on any device;
        1 <= Q <= 4096.  query_mask: [B, Q] or [Q], bool / integer, nonzero = valid -- HF's `query_mask`; masked logits are finfo(f32).min, as HF
        writes them.  Queries are normalised HF's way, q / (|q| + 1e-6); unit text rows are therefore normalised a second time, as in HF.

        Image-guided detection needs no other entry: `model.detect(img, model.embed_image_query(ex, boxes)[0][None])` is HF's
        `image_guided_detection` for one exemplar.  HF's post-processing is `PostProcess(confidence_threshold=t, iou_threshold=1.0)(pred_boxes, scores)`
        (the class is the arg-max query; an IoU threshold of 1 keeps everything, HF's `post_process_object_detection` has no NMS).

        Needs `set_logit_head` (RuntimeError otherwise).  Inference only; `forward_queries` is the gradient-recording form.  Runs the plain eval forward on the EVAL
        workspace behind a deferred optimizer tail (a pending training backward is not disturbed), in chunks of at most 32 images; the frozen-prefix
        cache is neither read nor written; `forward` and its outputs are untouched.  No host sync.

        objectness=True (OWLv2; needs `set_objectness_head`, RuntimeError otherwise) appends HF's `objectness_logits` f32 [B, P] to the result: the objectness
        head on each chunk's features, right behind its forward, with its two hidden layers in the eval workspace's box-head buffers (free by then): three
        launches per chunk and no allocation but the output.  Without the flag no launch and no bit changes, head set or not."""
        if self.logit_head is None:
            raise RuntimeError("detect: no logit head -- call model.set_logit_head(weights.hf_logit_head(hf_state_dict)) or load_model(..., logit_head=)")
        if objectness:
            self._need_objectness("detect")
        B, Q, shared = check_detect_args(self.cfg, pixel_values, query_embeds, query_mask)
        cfg, dev, P = self.cfg, self.device_, self.cfg.patches
        qe = torch.as_tensor(query_embeds).to(dev).contiguous()
        qm = None
        if query_mask is not None:
            qm = (torch.as_tensor(query_mask).to(dev) != 0).to(torch.uint8).contiguous()
        lh = self.logit_head
        self._wait_params()
        boxes = torch.empty(B, P, 4, dtype=torch.float32, device=dev)
        logits = torch.empty(B, P, Q, dtype=torch.float32, device=dev)
        scores = torch.empty(B, P, Q, dtype=torch.float32, device=dev) if return_scores else None
        obj = torch.empty(B, P, dtype=torch.float32, device=dev) if objectness else None
        keep = self.max_cached_batch_sizes          # (as _embed_image_query: no size is evicted by this call)
        self.max_cached_batch_sizes = max(1, int(keep)) + 2
        try:
            for a in range(0, B, EXEMPLAR_CHUNK):
                nb = min(EXEMPLAR_CHUNK, B - a)
                pb, _ = self._forward_impl(pixel_values[a:a + nb], save=False)
                ws = self._workspace(nb, train=False)
                if "logit_rowstats" not in ws:
                    ws["logit_rowstats"] = torch.zeros(nb * P, 2, dtype=torch.float32, device=dev)
                ops.class_logits(ws["e"], qe if shared else qe[a:a + nb], ws["feats"], lh["logit_shift.weight"], lh["logit_shift.bias"],
                                 lh["logit_scale.weight"], lh["logit_scale.bias"], nb, P, mask=None if qm is None else (qm if qm.dim() == 1 else qm[a:a + nb]),
                                 rowstats=ws["logit_rowstats"], logits=logits[a:a + nb], scores=scores[a:a + nb] if return_scores else False)
                if objectness:
                    self._objectness_on(ws["feats"], ws["hb0"], ws["hb1"], obj[a:a + nb], nb * P)
                boxes[a:a + nb].copy_(pb)
        finally:
            self.max_cached_batch_sizes = keep
        out = (boxes, logits, scores) if return_scores else (boxes, logits)
        return out + (obj,) if objectness else out

    @torch.no_grad()
    def detect_text(self, pixel_values, input_ids, text_tower, return_scores=False, shared=None, objectness=False):
        """`detect` on tokenised prompts, HF's `OwlViTForObjectDetection.forward`: input_ids [B Q, S] (HF's layout) or [B, Q, S], Q prompts per image that
        may differ per image, padded queries all-zero ids; or [Q, S] for one list shared by the batch.  A 2-D input whose row count is a multiple of B
        is read as [B Q, S] unless shared=True.  The embeddings are `text_tower.encode(ids)` (text.TextTower: the unit rows HF feeds its head), the
        mask is ids[..., 0] > 0 as in HF.  -> detect's result (objectness=True: with `objectness_logits` appended)."""
        embeds, mask = text_queries("detect_text", int(pixel_values.shape[0]), input_ids, text_tower, shared)
        return self.detect(pixel_values, embeds, mask, return_scores=return_scores, objectness=objectness)

    # -- open-vocabulary fine-tuning: the same head, gradient-recording ---------------------------------------------------------
    def _class_logits_on(self, ws, B, qe, qm):
        """HF's class head on a workspace's e / feats -> logits [B, P, Q]; (shift, scale) per row stay in ws["logit_rowstats"] for the adjoint."""
        lh, P = self.logit_head, self.cfg.patches
        if "logit_rowstats" not in ws:
            ws["logit_rowstats"] = torch.zeros(B * P, 2, dtype=torch.float32, device=self.device_)
        return ops.class_logits(ws["e"], qe, ws["feats"], lh["logit_shift.weight"], lh["logit_shift.bias"], lh["logit_scale.weight"], lh["logit_scale.bias"],
                                B, P, mask=qm, rowstats=ws["logit_rowstats"])[0]

    def forward_queries(self, pixel_values, query_embeds, query_mask=None, objectness=False):
        """The gradient-recording form of `detect`: -> (pred_boxes [B, P, 4] corners, logits [B, P, Q]) of HF's class head over the caller's queries,
        arguments as for `detect` (a bank per image [B, Q, Dt] or one shared [Q, Dt], an optional mask; masked logits are finfo(f32).min and pass no
        gradient -- select them out of the loss).  Needs `set_logit_head` (RuntimeError otherwise).

        With grad enabled the forward runs on the TRAINING workspace, pred_boxes carry the bits of `model(image)[0]`, and backward() accumulates into
        the model's trainable set -- any set `trainable=` accepts -- exactly as the bank path does (flat_grad, FusedAdamW, the deferred tail), through
        csrc/open_vocab_bwd.hip instead of the bank head's adjoint.  What is NOT trained: the learnable bank `queries` (it takes no part and gets no
        gradient), the four logit-head tensors unless set_logit_head(head, trainable=True) made them leaves (frozen buffers by default; the gradient
        passes through them to the features either way; trained, their gradients arrive as ordinary autograd gradients) and any text tower.  If
        `query_embeds.requires_grad` it receives its gradient as an ordinary autograd gradient (prompt tuning: the tensor is the caller's, stepped by
        any torch optimizer; under the deferred tail the caller's stream is ordered behind it).  As with `forward`, call backward() before the next
        recording forward at the same batch size (RuntimeError otherwise).  The loss over [B, P, Q] logits is
        `losses.OpenVocabLoss` (bipartite matching, sigmoid focal + L1 / GIoU, on device with no host sync), or any torch code of the caller's.

        Under no_grad it is `detect`.

        objectness=True (OWLv2; needs `set_objectness_head`) -> (pred_boxes, logits, objectness_logits [B, P]).  With grad enabled the head runs on the
        training workspace's features with activations of its own.  It reads them DETACHED, as HF does: nothing of it reaches the trunk or flat_grad.  A
        frozen head's result carries no grad_fn; a trainable head's (set_objectness_head(head, trainable=True)) is the output of
        autograd.OwlViTObjectnessFunction, whose backward writes the six leaves' gradients -- before, after or without the main backward, same bits -- and
        is held to the same rule: backward() before the next recording forward at this batch size."""
        if self.logit_head is None:
            raise RuntimeError("forward_queries: no logit head -- call model.set_logit_head(weights.hf_logit_head(hf_state_dict)) or load_model(..., logit_head=)")
        if objectness:
            self._need_objectness("forward_queries")
        B, Q, shared = check_detect_args(self.cfg, pixel_values, query_embeds, query_mask)
        qe = torch.as_tensor(query_embeds)
        head = [self.logit_head[k] for k in W.LOGIT_HEAD_KEYS if self.logit_head[k].requires_grad] if self.logit_head else []          # a trainable head's leaves
        obj_leaves = self.objectness_head_parameters() if objectness else []          # (a trainable objectness head alone is reason enough to record)
        need_grad = torch.is_grad_enabled() and (qe.requires_grad or bool(head) or bool(obj_leaves) or any(p.requires_grad for p in self.parameters()))
        if not need_grad:
            return self.detect(pixel_values, qe.detach(), query_mask, objectness=objectness)
        self._check_trainable_set()
        qe = qe.to(self.device_).contiguous()          # (autograd-recorded: the gradient finds its way back to the caller's tensor)
        qm = None
        if query_mask is not None:
            qm = (torch.as_tensor(query_mask).to(self.device_) != 0).to(torch.uint8).contiguous()
        from .autograd import OwlViTObjectnessFunction, OwlViTQueryFunction
        if head and len(head) != 4:
            raise RuntimeError("forward_queries: the four logit-head tensors train together or not at all (set_logit_head(head, trainable=True))")
        out = OwlViTQueryFunction.apply(self, pixel_values, qe, qm, *[self._byname[n] for n in self.flat_offsets], *head)
        if not objectness:
            return out
        leaves = obj_leaves
        if leaves and len(leaves) != 6:
            raise RuntimeError("forward_queries: the six objectness-head tensors train together or not at all (set_objectness_head(head, trainable=True))")
        if leaves:
            return out + (OwlViTObjectnessFunction.apply(self, B, *leaves),)
        with torch.no_grad():
            return out + (self._objectness_train_forward(B),)

    def forward_text(self, pixel_values, input_ids, text_tower, shared=None, objectness=False):
        """`forward_queries` on tokenised prompts, input_ids laid out as for `detect_text`.  The text tower stays forward-only: its embeddings are
        detached constants (nothing is trained in it)."""
        with torch.no_grad():
            embeds, mask = text_queries("forward_text", int(pixel_values.shape[0]), input_ids, text_tower, shared)
        return self.forward_queries(pixel_values, embeds.detach(), mask, objectness=objectness)


def text_queries(who, B, input_ids, text_tower, shared=None):
    """The id layouts of detect_text / forward_text -> (embeds [B, Q, Dt] or [Q, Dt] = text_tower.encode(ids), mask = ids[..., 0] > 0 of the same
    leading shape).  ValueError (prefixed `who`) names the layouts."""
    ids = torch.as_tensor(np.asarray(input_ids) if not torch.is_tensor(input_ids) else input_ids)
    if ids.dim() == 3:
        if ids.shape[0] != B:
            raise ValueError(f"{who}: input_ids must be [{B}, Q, S], [{B} Q, S] or [Q, S], got {tuple(ids.shape)}")
        shape = (B, int(ids.shape[1]))
    elif ids.dim() == 2:
        if shared is None:
            shared = ids.shape[0] % B != 0
        if not shared and ids.shape[0] % B:
            raise ValueError(f"{who}: input_ids [{ids.shape[0]}, S] is not [{B} Q, S] for a batch of {B} images")
        shape = (int(ids.shape[0]),) if shared else (B, int(ids.shape[0]) // B)
    else:
        raise ValueError(f"{who}: input_ids must be [{B}, Q, S], [{B} Q, S] or [Q, S], got {tuple(ids.shape)}")
    flat = ids.reshape(-1, ids.shape[-1])
    embeds = text_tower.encode(flat).reshape(*shape, -1)
    mask = (flat[:, 0] > 0).reshape(*shape)
    return embeds, mask


def check_detect_args(cfg, pixel_values, query_embeds, query_mask=None):
    """Host-side validation of OwlViT.detect's arguments (shapes and dtypes only: no device is touched) -> (B, Q, shared bank?).  ValueError names
    the expected shape."""
    if not hasattr(pixel_values, "shape") or len(pixel_values.shape) != 4 or tuple(pixel_values.shape[1:]) != (3, *cfg.image_hw) \
            or pixel_values.shape[0] < 1:
        raise ValueError(f"detect: pixel_values must be [B, 3, {cfg.image_hw[0]}, {cfg.image_hw[1]}] with B >= 1, got {tuple(getattr(pixel_values, 'shape', ()))}")
    B, Dt = int(pixel_values.shape[0]), cfg.text_dim
    qe = torch.as_tensor(query_embeds)
    if qe.dim() not in (2, 3) or qe.shape[-1] != Dt or (qe.dim() == 3 and qe.shape[0] != B):
        raise ValueError(f"detect: query_embeds must be [{B}, Q, {Dt}] or [Q, {Dt}], got {tuple(qe.shape)}")
    if qe.dtype != torch.float32:
        raise ValueError(f"detect: query_embeds must be float32 [{B}, Q, {Dt}] or [Q, {Dt}], got {qe.dtype}")
    Q = int(qe.shape[-2])
    if not 1 <= Q <= ops.CLASS_LOGITS_MAX_QUERIES:
        raise ValueError(f"detect: query_embeds must be [{B}, Q, {Dt}] or [Q, {Dt}] with 1 <= Q <= {ops.CLASS_LOGITS_MAX_QUERIES}, got Q = {Q}")
    if query_mask is not None:
        qm = torch.as_tensor(query_mask)
        if tuple(qm.shape) not in ((B, Q), (Q,)):
            raise ValueError(f"detect: query_mask must be [{B}, {Q}] or [{Q}], got {tuple(qm.shape)}")
        if qm.dtype.is_floating_point or qm.dtype.is_complex:
            raise ValueError(f"detect: query_mask must be bool or integer [{B}, {Q}] or [{Q}] (nonzero = valid), got {qm.dtype}")
    return B, Q, qe.dim() == 2


EXEMPLAR_CHUNK = 32          # images per forward of embed_image_query and detect


def exemplar_slots(class_ids, n_classes):
    """The slot rule of set_queries_from_exemplars, a pure host function: -> 3 C lists of exemplar indices (ascending), list 3 c + s = the members of slot
    s of class c.  With the exemplars of class c numbered k = 0, 1, ... in the order given, slot s takes {k : k % 3 == s} when that set is not empty and
    exemplar s % n_c otherwise; the three lists of a class without exemplars are empty (its rows are kept)."""
    per = [[] for _ in range(int(n_classes))]
    for n, c in enumerate(class_ids):
        per[int(c)].append(n)
    table = []
    for mem in per:
        for s in range(3):
            table.append([] if not mem else (mem[s::3] or [mem[s % len(mem)]]))
    return table


def slots_csr(table):
    """A slot table (exemplar_slots) as the CSR arrays owl_query_bank_fill takes: (row_ptr int32 [rows + 1], members int32, at least one entry)."""
    row_ptr = np.zeros(len(table) + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum([len(m) for m in table])
    members = np.asarray([n for m in table for n in m] or [0], dtype=np.int32)
    return row_ptr, members


def check_exemplars(class_ids, query_boxes, n_images, n_classes):
    """Host-side validation of an exemplar set -> the class ids as a list of int.  Raises ValueError naming the exemplar and its class."""
    ids = [int(c) for c in (class_ids.tolist() if hasattr(class_ids, "tolist") else class_ids)]
    if len(ids) != n_images or not ids:
        raise ValueError(f"exemplars: {n_images} images for {len(ids)} class ids (one class id per example image, at least one)")
    for n, c in enumerate(ids):
        if not 0 <= c < n_classes:
            raise ValueError(f"exemplars: exemplar {n} has class {c}, outside [0, {n_classes})")
    if query_boxes is not None:
        qb = torch.as_tensor(query_boxes, dtype=torch.float32).cpu()
        if tuple(qb.shape) != (n_images, 4):
            raise ValueError(f"exemplars: query_boxes must be [{n_images}, 4] normalised corners (x0, y0, x1, y1), got {tuple(qb.shape)}")
        for n, (x0, y0, x1, y1) in enumerate(qb.tolist()):
            if not (x0 < x1 and y0 < y1):          # (a NaN fails too)
                raise ValueError(f"exemplars: exemplar {n} (class {ids[n]}) has query box ({x0:g}, {y0:g}, {x1:g}, {y1:g}): corners need x0 < x1 and y0 < y1")
    return ids


def load_model(labelmap, device="cuda", arch: str = "owlvit-base-patch32", seed: int = 1234, state=None, *,
               prompt_ids=None, text_state=None, vocab=None, merges=None, trainable=None, image_size=None, exemplars=None, logit_head=None,
               logit_head_trainable=False, objectness_head=None, objectness_head_trainable=False):
    """ref src/models.py:149-191.  The reference downloads `google/owlvit-base-patch32` and runs the
    CLIP text tower once to initialise the query bank; neither box has network access, so weights
    come from `state` (name -> array, reference parameter names) or, by default, the deterministic
    random set (weights.make_weights).  The freeze rule is applied by construction (trainable
    tensors live in the flat bucket with requires_grad=True; everything else is frozen).

    `prompt_ids` ([3C, S] CLIP token ids of `[label, "a photo of "+label, "a "+label+" in an environment"]`
    per class, class-major, ref models.py:155-159 -- tokenised by the caller's processor) switches on the
    reference's query-bank initialisation: the text tower (text.TextTower; weights from `text_state`, HF names
    `text_model.*` / `text_projection.weight`, or the deterministic random set) runs once on the device and its
    L2-normalised `text_embeds` become `queries` (ref models.py:161-169).

    `vocab` / `merges` (paths of the CLIP `vocab.json` / `merges.txt` every OWL-ViT checkpoint carries -- a download neither box can make, so they
    are not shipped): the three prompts per label are built and tokenised HERE exactly as the reference does (ref models.py:155-166 via
    tokenizer.ClipBPE, id for id `transformers.CLIPTokenizer`), i.e. the unchanged `load_model(labelmap, device)` call of ref main.py:42 plus the two
    paths gives the reference's query bank.

    `trainable` (None = the reference's freeze rule): the substring list of that rule, as a user of the reference would edit it -- see OwlViT.

    `image_size` (None = the architecture's): the input size the model is built for, an int (square) or a pair (height, width); each side a multiple of
    the patch size, at most 8192 patches and 256 patches per side
    (HF's `interpolate_pos_encoding=True`, HF5:296-332).  The native grid of the position table is read off `state`'s table (a checkpoint's, through
    weights.from_hf_state_dict) or is the architecture's; the parameter keeps that shape and the embeddings read a bicubic resample of it, so
    state dicts and FusedAdamW states move freely between sizes.  At the native size nothing changes.

    `exemplars` (None = nothing new runs or is allocated): `(pixel_values, class_ids[, query_boxes])`, annotated example images at the model's input size --
    the image prior for classes a short prompt does not describe.  Applied after construction, hence after the text initialisation when `prompt_ids=` /
    `vocab=` is given too (OwlViT.set_queries_from_exemplars): classes with exemplars take the image prior, the others keep the text (or random) one.

    `logit_head` (None = none is set): weights.hf_logit_head(sd), HF's `class_head.logit_shift / logit_scale` -- what zero-shot inference
    (OwlViT.detect / detect_text) needs beside the vision path.  Frozen buffers outside the parameters: see OwlViT.set_logit_head.
    `logit_head_trainable=True` makes them four leaf tensors that `forward_queries`' backward gives gradients (still outside the parameters; stepped
    by the caller's torch optimizer over `model.logit_head_parameters()`).

    `objectness_head` (None = none is set): weights.hf_objectness_head(sd), the six `objectness_head.*` tensors of an OWLv2 checkpoint -- what
    `detect(..., objectness=True)` needs; `objectness_head_trainable=True` makes them six leaf tensors (OwlViT.set_objectness_head)."""
    n_classes = len(labelmap)
    cfg = get_config(arch, n_classes=n_classes)
    g0 = table_grid(np.asarray(state[_POS]).shape[0]) if (state is not None and _POS in state) else cfg.grid
    if image_size is not None or g0 != cfg.grid:
        S = cfg.image_size if image_size is None else (tuple(int(v) for v in image_size) if isinstance(image_size, (tuple, list)) else int(image_size))
        g = check_image_size(S, cfg.patch_size, g0 * g0 + 1)
        cfg = cfg.replace(image_size=S, pos_grid=0 if g in (g0, (g0, g0)) else g0)
    if (vocab is None) != (merges is None):
        raise ValueError("load_model: vocab= and merges= go together (the CLIP vocab.json and merges.txt)")
    if vocab is not None:
        if prompt_ids is not None:
            raise ValueError("load_model: give either prompt_ids= or vocab= / merges=")
        from .config import get_text_config
        from .tokenizer import ClipBPE, label_prompts
        lm = labelmap if hasattr(labelmap, "values") else {i: l for i, l in enumerate(labelmap)}
        prompt_ids = ClipBPE(vocab, merges, max_length=get_text_config(arch).max_pos)(label_prompts(lm))
    if state is None:
        state = W.make_weights(cfg, seed)
    if prompt_ids is not None:
        from .config import get_text_config
        from .text import TextTower
        ids = np.asarray(prompt_ids.cpu() if torch.is_tensor(prompt_ids) else prompt_ids)
        if ids.ndim == 3:                         # processor(text=[to_encode]) yields [1, 3C, S]
            ids = ids[0]
        if ids.shape[0] != cfg.queries:
            raise ValueError(f"load_model: expected {cfg.queries} prompts (3 per class), got {ids.shape[0]}")
        tower = TextTower(get_text_config(arch), text_state, device, seed)
        state = OrderedDict(state)
        state["queries"] = tower.query_bank(ids).cpu().numpy()
        del tower
    model = OwlViT(cfg, state, device, trainable=trainable)
    if exemplars is not None:
        if not 2 <= len(exemplars) <= 3:
            raise ValueError("load_model: exemplars= is (pixel_values, class_ids) or (pixel_values, class_ids, query_boxes)")
        model.set_queries_from_exemplars(*exemplars)
    if logit_head is not None:
        model.set_logit_head(logit_head, trainable=logit_head_trainable)
    if objectness_head is not None:
        model.set_objectness_head(objectness_head, trainable=objectness_head_trainable)
    return model
