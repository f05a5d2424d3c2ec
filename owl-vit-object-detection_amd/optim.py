"""Fused AdamW over the model's flat trainable bucket.

Drop-in for the reference's optimizer (ref main.py:56-60: `torch.optim.AdamW(model.parameters(), lr,
weight_decay)`, single param group -- weight decay also hits LayerNorm affine, biases and the query bank):
same constructor keywords, `zero_grad()` / `step()`.  One HIP kernel touches (param, grad, m, v) once and
refreshes the bf16 compute copy.  torch.optim.AdamW on `model.parameters()` also works (the parameters are
ordinary f32 leaves); this class is the fast path.

It is a `torch.optim.Optimizer` over the model's trainable parameters, so `torch.optim.lr_scheduler.*` drive it:
`step()` reads `lr` / `weight_decay` from `param_groups` on every call.  Two keyword-only additions stay on the fused
path: `param_groups=` (per-group `lr` / `weight_decay`, e.g. no decay for LayerNorm affines, biases and the query
bank) and `max_norm=` (global L2 gradient-norm clipping, `torch.nn.utils.clip_grad_norm_`'s formula, without a sync).
With one group and no clipping the step is the one-group kernel, unchanged.
"""
import math

import torch

from . import _lib, ops
from .autograd import _attach_grads, _grads_attached

MAX_SEGMENTS = 32          # rows of the (end_offset, lr, weight_decay) table owl_adamw_step_grouped takes by value


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, overlap: bool = False, param_groups=None,
                 max_norm=None):
        """overlap=True (keyword-only addition): backward + this step run on the model's tail stream under the NEXT forward's frozen prefix
        (models.OwlViT.overlap_tail) -- bitwise the in-line schedule.  The model's own forward / backward / zero_grad / state_dict order
        themselves behind the deferred tail; anything else that reads `p.grad` or the parameters calls `model.finish()` first (and finds the
        gradient bucket already zeroed after a step: the zeroing of the next `zero_grad()` is part of the tail).

        param_groups=[{"params": [parameters or dotted names], "lr": ..., "weight_decay": ...}, ...]: the trainable tensors not listed form the
        default group (`lr`, `weight_decay` of the constructor), which comes first in `self.param_groups`.  `betas` and `eps` are global.
        max_norm: clip the global L2 norm of the (scaled, under data parallel: averaged) gradient to it; `last_grad_norm` is the device tensor that
        receives the norm before clipping -- reading it is the caller's sync."""
        self.model = model
        if overlap:
            model.overlap_tail = True
        if max_norm is not None and not (float(max_norm) > 0 and math.isfinite(float(max_norm))):
            raise ValueError(f"FusedAdamW: max_norm must be None (no clipping) or a positive finite number, got {max_norm!r}")
        self.max_norm = None if max_norm is None else float(max_norm)
        groups, self._segments = self._plan(model, param_groups)
        self._built = False
        super().__init__(groups, dict(lr=float(lr), betas=tuple(betas), eps=float(eps), weight_decay=float(weight_decay)))
        self._built = True
        self.exp_avg = torch.zeros_like(model.flat_param)
        self.exp_avg_sq = torch.zeros_like(model.flat_param)
        self.step_count = 0
        self.grad_scale = 1.0          # set to 1/world_size by the data-parallel wrapper
        # scratch of the clipped step (one f64 partial sum of squares per workgroup) and the norm it reports: allocated once, here
        nbytes = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_grad_norm_workspace_bytes", model.flat_numel, nbytes)
        self._norm_ws = torch.zeros(int(nbytes.item()) // 8, dtype=torch.float64, device=model.flat_param.device)
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=model.flat_param.device)
        # host side of the segment table: the end offsets are fixed, lr / weight_decay are refilled from param_groups by every step
        self._seg_end = torch.tensor([end for end, _ in self._segments], dtype=torch.int64)
        self._seg_lr = torch.zeros(len(self._segments), dtype=torch.float32)
        self._seg_wd = torch.zeros(len(self._segments), dtype=torch.float32)

    @staticmethod
    def _plan(model, user_groups):
        """-> (param group dicts for torch.optim.Optimizer, [(end_offset, group index)] = runs of adjacent tensors of one group in bucket order)."""
        names = list(model.flat_offsets)
        by_id = {id(model.p(n)): n for n in names}
        all_names = {id(p): n for n, p in model.named_parameters()}
        owner = {}
        listed = []
        for gi, grp in enumerate(user_groups or []):
            if not isinstance(grp, dict) or "params" not in grp:
                raise ValueError(f"FusedAdamW: param_groups[{gi}] must be a dict with a `params` list")
            members = []
            for t in grp["params"]:
                if isinstance(t, str):
                    if t not in model.flat_offsets:
                        raise ValueError(f"FusedAdamW: param_groups[{gi}] names `{t}`, which is "
                                         + ("a frozen tensor" if t in all_names.values() else "not a parameter of the model"))
                    name = t
                elif id(t) in by_id:
                    name = by_id[id(t)]
                elif id(t) in all_names:
                    raise ValueError(f"FusedAdamW: param_groups[{gi}] holds `{all_names[id(t)]}`, which is a frozen tensor")
                else:
                    raise ValueError(f"FusedAdamW: param_groups[{gi}] holds a foreign tensor of shape {tuple(getattr(t, 'shape', ()))}: not a "
                                     "trainable parameter of the model")
                if name in owner:
                    raise ValueError(f"FusedAdamW: `{name}` is in two parameter groups (param_groups[{owner[name]}] and param_groups[{gi}])")
                owner[name] = gi
                members.append(name)
            if not members:
                raise ValueError(f"FusedAdamW: param_groups[{gi}] lists no parameter")
            for key in grp:
                if key in ("betas", "eps"):
                    raise ValueError(f"FusedAdamW: per-group `{key}` (param_groups[{gi}], `{members[0]}` ...): betas and eps are global to the fused step")
                if key not in ("params", "lr", "weight_decay"):
                    raise ValueError(f"FusedAdamW: param_groups[{gi}] (`{members[0]}` ...) has the unknown key `{key}`")
            listed.append(dict({k: float(v) for k, v in grp.items() if k != "params"}, params=[model.p(n) for n in names if owner.get(n) == gi]))
        rest = [n for n in names if n not in owner]
        groups = ([dict(params=[model.p(n) for n in rest])] if rest else []) + listed
        shift = 1 if rest else 0
        segments = []
        for k, n in enumerate(names):
            gi = owner[n] + shift if n in owner else 0
            end = model.flat_offsets[names[k + 1]] if k + 1 < len(names) else model.flat_numel
            if segments and segments[-1][1] == gi:
                segments[-1] = (end, gi)
            else:
                if len(segments) == MAX_SEGMENTS:
                    raise ValueError(f"FusedAdamW: more than {MAX_SEGMENTS} segments after merging adjacent tensors of one group (the next one would start at "
                                     f"`{n}`): group tensors that are neighbours in the bucket (model.flat_offsets) together")
                segments.append((end, gi))
        return groups, segments

    def add_param_group(self, param_group):
        if self._built:
            raise ValueError("FusedAdamW: the groups are fixed at construction (param_groups=): the segment table of the fused step is built from them")
        super().add_param_group(param_group)

    # the one-group surface: `lr` / `weight_decay` are those of the first (the default) group; `betas` / `eps` are global
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, x):
        self.param_groups[0]["lr"] = float(x)

    @property
    def weight_decay(self):
        return self.param_groups[0]["weight_decay"]

    @weight_decay.setter
    def weight_decay(self, x):
        self.param_groups[0]["weight_decay"] = float(x)

    @property
    def betas(self):
        return self.param_groups[0]["betas"]

    @betas.setter
    def betas(self, x):
        for g in self.param_groups:
            g["betas"] = tuple(x)

    @property
    def eps(self):
        return self.param_groups[0]["eps"]

    @eps.setter
    def eps(self, x):
        for g in self.param_groups:
            g["eps"] = float(x)

    def _attach(self):
        """Re-attach detached `.grad` views (nn.Module.zero_grad(set_to_none=True) drops them).  Attaching zero-fills the bucket on the CURRENT
        stream: behind a deferred tail that may still be reading / zeroing it."""
        m = self.model
        if not _grads_attached(m):          # (detached, or foreign .grad tensors: re-attaching zero-fills / copies into the bucket)
            self._sync_tail()
            _attach_grads(m)

    def _sync_tail(self):
        """Order the current stream behind everything the tail stream holds (deferred backward / all-reduce / AdamW / zeroing)."""
        m = self.model
        m._wait_params()
        if m.flat_param.is_cuda and getattr(m, "_tail_stream_", None) is not None and torch.cuda.current_stream() != m._tail_stream_:
            torch.cuda.current_stream().wait_stream(m._tail_stream_)

    def zero_grad(self, set_to_none: bool = False):
        self._attach()
        if getattr(self.model, "_grad_clean", False):
            return                       # a deferred step (ddp.DataParallel(overlap=True)) already zeroed the bucket on its stream
        self.model._wait_params()
        self.model.flat_grad.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        m = self.model
        self._attach()
        m._grad_clean = False
        self.step_count += 1
        deferred = getattr(m, "overlap_tail", False) and m.flat_param.is_cuda and torch.cuda.current_stream() != m._tail_stream
        if deferred:
            # the backward of this step is (or may be) still running on the tail stream: the update and the zeroing of the bucket follow it there
            ts = m._tail_stream
            ts.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(ts):
                self._launch()
                m.flat_grad.zero_()               # the next zero_grad(), done where nothing races with the reads above
                ev = torch.cuda.Event()
                ev.record(ts)
            m._param_event = ev
            m._grad_clean = True
        else:
            self._launch()
        m._mark_bf16_current()          # one-shot token for the next forward (models.OwlViT.__init__)
        return loss

    def _launch(self):
        m, groups = self.model, self.param_groups
        g0 = groups[0]
        betas, eps = g0["betas"], g0["eps"]
        if len(groups) == 1 and self.max_norm is None:
            _lib.call("owl_adamw_step", ops.stream(), m.flat_param, m.flat_grad, self.exp_avg, self.exp_avg_sq, m.flat_bf16,
                      m.flat_numel, float(g0["lr"]), betas[0], betas[1], eps, float(g0["weight_decay"]), self.step_count,
                      float(self.grad_scale))
            return
        for k, g in enumerate(groups):
            if tuple(g["betas"]) != tuple(betas) or g["eps"] != eps:
                raise ValueError(f"FusedAdamW: param_groups[{k}] has its own betas / eps: they are global to the fused step")
        for s, (_, gi) in enumerate(self._segments):
            self._seg_lr[s] = float(groups[gi]["lr"])
            self._seg_wd[s] = float(groups[gi]["weight_decay"])
        clip = self.max_norm is not None
        if clip:
            _lib.call("owl_grad_sumsq", ops.stream(), m.flat_grad, m.flat_numel, self._norm_ws)
        # (the scalar lr / weight_decay arguments only stand in for a null table)
        _lib.call("owl_adamw_step_grouped", ops.stream(), m.flat_param, m.flat_grad, self.exp_avg, self.exp_avg_sq, m.flat_bf16,
                  m.flat_numel, float(g0["lr"]), betas[0], betas[1], eps, float(g0["weight_decay"]), self.step_count, float(self.grad_scale),
                  self._seg_end, self._seg_lr, self._seg_wd, len(self._segments), self.max_norm if clip else 0.0,
                  self._norm_ws if clip else None, self.last_grad_norm if clip else None)

    def state_dict(self):
        self._sync_tail()               # a deferred step may still be writing the moments on the tail stream
        keys = ("lr", "weight_decay", "initial_lr")          # (`initial_lr`: set by a torch LR scheduler at its construction)
        return dict(step=self.step_count, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr=self.lr, betas=self.betas,
                    eps=self.eps, weight_decay=self.weight_decay, max_norm=self.max_norm,
                    layout=list(self.model.flat_offsets.items()),          # (the bucket's tensors and offsets: the moments are meaningless under another trainable set)
                    groups=[{k: g[k] for k in keys if k in g} for g in self.param_groups])

    def load_state_dict(self, sd):
        """Moments and step count; the groups' lr / weight_decay / initial_lr and max_norm where the dict has them (one written before it had: not)."""
        self._sync_tail()
        mine = list(self.model.flat_offsets.items())
        theirs = [tuple(x) for x in sd["layout"]] if "layout" in sd else None
        if (theirs is not None and theirs != mine) or tuple(sd["exp_avg"].shape) != tuple(self.exp_avg.shape):
            other = "" if theirs is None else f" (its bucket holds {len(theirs)} tensors, e.g. `{(sorted(set(n for n, _ in theirs) - set(self.model.flat_offsets)) or [theirs[0][0]])[0]}`)"
            raise ValueError(f"FusedAdamW.load_state_dict: this state dict was written for a different trainable set{other}: its moments are laid out for a bucket of "
                             f"{sd['exp_avg'].numel()} elements, this model's bucket ({len(mine)} tensors, trainable= of its construction) has {self.exp_avg.numel()}")
        if "groups" in sd and len(sd["groups"]) != len(self.param_groups):
            raise ValueError(f"FusedAdamW.load_state_dict: the dict has {len(sd['groups'])} parameter groups, this optimizer {len(self.param_groups)}")
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        for g, saved in zip(self.param_groups, sd.get("groups", [])):
            g.update(saved)
        if "max_norm" in sd:
            self.max_norm = sd["max_norm"]
