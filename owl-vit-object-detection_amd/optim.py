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

`ema_decay=` (keyword-only) keeps an exponential moving average of the trainable bucket -- one more f32 array of `flat_numel` elements, updated inside
the step's own pass -- and `with optimizer.ema_weights():` evaluates and exports with it.  `ModelEMA` is the same average for loops that keep
`torch.optim.AdamW`: one launch after the foreign step, the same bits.
"""
import contextlib
import math
import struct

import torch

from . import _lib, ops
from .autograd import _attach_grads, _grads_attached

MAX_SEGMENTS = 32          # rows of the (end_offset, lr, weight_decay) table owl_adamw_step_grouped takes by value


def ema_decay_at(step: int, decay: float, warmup: bool = True) -> float:
    """Decay of update number `step` (1-based).  With warm-up min(decay, (1 + step) / (10 + step)) -- 2/11 at the first update, so the average leaves
    its seed quickly, and `decay` from the step where (1 + step) / (10 + step) reaches it; without warm-up `decay`.  A pure host function of its
    arguments: nothing is read from the device."""
    step, decay = int(step), float(decay)
    if step < 1:
        raise ValueError(f"ema_decay_at: step is the 1-based count of the update, got {step}")
    return min(decay, (1 + step) / (10 + step)) if warmup else decay


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def ema_coefficients(decay: float):
    """-> (d, w) as the kernels take them: d = `decay` rounded to f32, w = 1 - d taken in double from that f32 d and rounded to f32."""
    d = _f32(decay)
    return d, _f32(1.0 - d)


def _check_decay(who, decay):
    if not 0.0 <= float(decay) <= 1.0:          # (a NaN fails both comparisons)
        raise ValueError(f"{who}: the EMA decay must lie in [0, 1], got {decay!r}")
    return float(decay)


def _order_behind_tail(m):
    """Order the current stream behind everything the model's tail stream holds (deferred backward / all-reduce / AdamW / zeroing)."""
    m._wait_params()
    if m.flat_param.is_cuda and getattr(m, "_tail_stream_", None) is not None and torch.cuda.current_stream() != m._tail_stream_:
        torch.cuda.current_stream().wait_stream(m._tail_stream_)


class _EmaState:
    """The average and its eval scope, shared by FusedAdamW(ema_decay=) and ModelEMA.  `self.model`, `self.ema` (None = off), `self.ema_decay`,
    `self.ema_warmup` and `self.ema_updates` are the owner's."""
    _ema_stash = None          # the raw iterate while the scope holds the averaged weights; allocated at the first entry
    _ema_active = False

    def _next_ema_coefficients(self):
        """(d, w) of the update about to be launched; counts it."""
        self.ema_updates += 1
        return ema_coefficients(ema_decay_at(self.ema_updates, self.ema_decay, self.ema_warmup))

    def _refuse_in_scope(self, what):
        if self._ema_active:
            raise RuntimeError(f"{type(self).__name__}.{what} inside `with ema_weights():` -- the bucket holds the averaged weights, the raw iterate is "
                               "stashed: leave the scope first")

    def ema_named(self):
        """{name: view into `ema`} with the parameters' shapes, in `model.flat_offsets` order."""
        if self.ema is None:
            raise ValueError(f"{type(self).__name__}.ema_named: no average is kept (ema_decay=None)")
        m = self.model
        return {n: self.ema[o: o + m.p(n).numel()].view(m.p(n).shape) for n, o in m.flat_offsets.items()}

    @contextlib.contextmanager
    def ema_weights(self):
        """Eval / export scope: inside it the model's trainable tensors hold the average -- `model(...)` and `model.state_dict()` see it -- and on exit
        the raw iterate is back, bit for bit.  Two copies of the bucket each way, ordered behind a deferred tail.  The copies go through
        `flat_param.copy_`, so the bucket's version counter moves and the next forward recasts the bf16 copy by itself; frozen tensors are not
        touched, so the frozen-prefix cache and the resampled position table of a frozen embedding stay valid."""
        if self.ema is None:
            raise ValueError(f"{type(self).__name__}.ema_weights: no average is kept (ema_decay=None)")
        self._refuse_in_scope("ema_weights() (a nested scope)")
        m = self.model
        _order_behind_tail(m)
        with torch.no_grad():
            if self._ema_stash is None:
                self._ema_stash = torch.empty_like(m.flat_param)
            self._ema_stash.copy_(m.flat_param)
            m.flat_param.copy_(self.ema)
        self._ema_active = True
        m._ema_scope = True          # (models.OwlViT.set_queries_from_exemplars refuses to write the bank while it holds the average)
        try:
            yield m
        finally:
            self._ema_active = False
            m._ema_scope = False
            with torch.no_grad():
                m.flat_param.copy_(self._ema_stash)

    def _ema_state_dict(self):
        return dict(ema=self.ema, ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, ema_updates=self.ema_updates)

    def _ema_load(self, sd):
        """A dict with the average restores it (and its decay, warm-up flag and count); one without re-seeds it from the current parameters, count 0."""
        if self.ema is None:
            return
        if "ema" in sd:
            if tuple(sd["ema"].shape) != tuple(self.ema.shape):
                raise ValueError(f"{type(self).__name__}.load_state_dict: the dict's average has {sd['ema'].numel()} elements, this model's bucket {self.ema.numel()}")
            self.ema.copy_(sd["ema"])
            self.ema_decay = _check_decay(type(self).__name__ + ".load_state_dict", sd.get("ema_decay", self.ema_decay))
            self.ema_warmup = bool(sd.get("ema_warmup", self.ema_warmup))
            self.ema_updates = int(sd.get("ema_updates", 0))
        else:
            self.ema.copy_(self.model.flat_param.detach())
            self.ema_updates = 0


class FusedAdamW(_EmaState, torch.optim.Optimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, overlap: bool = False, param_groups=None,
                 max_norm=None, ema_decay=None, ema_warmup: bool = True):
        """overlap=True (keyword-only addition): backward + this step run on the model's tail stream under the NEXT forward's frozen prefix
        (models.OwlViT.overlap_tail) -- bitwise the in-line schedule.  The model's own forward / backward / zero_grad / state_dict order
        themselves behind the deferred tail; anything else that reads `p.grad` or the parameters calls `model.finish()` first (and finds the
        gradient bucket already zeroed after a step: the zeroing of the next `zero_grad()` is part of the tail).

        param_groups=[{"params": [parameters or dotted names], "lr": ..., "weight_decay": ...}, ...]: the trainable tensors not listed form the
        default group (`lr`, `weight_decay` of the constructor), which comes first in `self.param_groups`.  `betas` and `eps` are global.
        max_norm: clip the global L2 norm of the (scaled, under data parallel: averaged) gradient to it; `last_grad_norm` is the device tensor that
        receives the norm before clipping -- reading it is the caller's sync.
        ema_decay (None = off: nothing is allocated or launched for it): `self.ema`, one f32 array of `model.flat_numel` elements seeded with the
        parameters, follows every step as ema <- d ema + (1 - d) p with d = ema_decay_at(update count, ema_decay, ema_warmup), inside the step's own
        pass and on the stream the step runs on.  `ema_named()` views it per tensor, `ema_updates` counts, `with optimizer.ema_weights():` evaluates
        with it.  Frozen tensors never change and have no average.  Under data parallel every rank computes the same bits: no collective."""
        self.model = model
        self.ema_decay = None if ema_decay is None else _check_decay("FusedAdamW", ema_decay)
        self.ema_warmup = bool(ema_warmup)
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
        self.ema, self.ema_updates = None, 0
        if self.ema_decay is not None:
            _order_behind_tail(model)
            self.ema = model.flat_param.detach().clone()
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
        _order_behind_tail(self.model)

    def zero_grad(self, set_to_none: bool = False):
        self._refuse_in_scope("zero_grad()")
        self._attach()
        if getattr(self.model, "_grad_clean", False):
            return                       # a deferred step (ddp.DataParallel(overlap=True)) already zeroed the bucket on its stream
        self.model._wait_params()
        self.model.flat_grad.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        self._refuse_in_scope("step()")
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
        if len(groups) == 1 and self.max_norm is None and self.ema is None:
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
        args = (ops.stream(), m.flat_param, m.flat_grad, self.exp_avg, self.exp_avg_sq, m.flat_bf16,
                m.flat_numel, float(g0["lr"]), betas[0], betas[1], eps, float(g0["weight_decay"]), self.step_count, float(self.grad_scale),
                self._seg_end, self._seg_lr, self._seg_wd, len(self._segments), self.max_norm if clip else 0.0,
                self._norm_ws if clip else None, self.last_grad_norm if clip else None)
        if self.ema is None:
            _lib.call("owl_adamw_step_grouped", *args)
        else:          # the same step with the average updated from the parameter it leaves behind, in the same pass (the one-group, unclipped case too)
            _lib.call("owl_adamw_step_ema", *args, self.ema, *self._next_ema_coefficients())

    def state_dict(self):
        self._sync_tail()               # a deferred step may still be writing the moments on the tail stream
        keys = ("lr", "weight_decay", "initial_lr")          # (`initial_lr`: set by a torch LR scheduler at its construction)
        return dict(**(self._ema_state_dict() if self.ema is not None else {}), step=self.step_count, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, lr=self.lr, betas=self.betas,
                    eps=self.eps, weight_decay=self.weight_decay, max_norm=self.max_norm,
                    layout=list(self.model.flat_offsets.items()),          # (the bucket's tensors and offsets: the moments are meaningless under another trainable set)
                    groups=[{k: g[k] for k in keys if k in g} for g in self.param_groups])

    def load_state_dict(self, sd):
        """Moments and step count; the groups' lr / weight_decay / initial_lr and max_norm where the dict has them (one written before it had: not).
        The average (`ema`, `ema_decay`, `ema_warmup`, `ema_updates`; `state_dict()` carries them when `ema_decay` is set): a dict WITHOUT them,
        loaded into an optimizer that keeps an average, re-seeds the average from the current parameters and sets its count to 0 -- load the model
        first; a dict WITH them, loaded into an optimizer without `ema_decay`, has them ignored."""
        self._refuse_in_scope("load_state_dict()")
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
        self._ema_load(sd)


class ModelEMA(_EmaState):
    """FusedAdamW(ema_decay=)'s average for a loop that keeps another optimizer (`torch.optim.AdamW(model.parameters())`): call `update()` after
    every `optimizer.step()`.  Same decay rule (`ema_decay_at`), same eval scope (`with ema.ema_weights():`), and -- fed the same parameters -- the same
    bits as the fused path: the fused step applies the very expression `owl_ema_update` does to the parameter it has just computed."""

    def __init__(self, model, decay, warmup: bool = True):
        self.model = model
        self.ema_decay = _check_decay("ModelEMA", decay)
        self.ema_warmup = bool(warmup)
        _order_behind_tail(model)
        self.ema = model.flat_param.detach().clone()
        self.ema_updates = 0

    @torch.no_grad()
    def update(self):
        """One launch over the bucket, on the current stream, behind a deferred tail's parameter event."""
        self._refuse_in_scope("update()")
        m = self.model
        m._wait_params()
        _lib.call("owl_ema_update", ops.stream(), self.ema, m.flat_param, m.flat_numel, *self._next_ema_coefficients())

    def state_dict(self):
        _order_behind_tail(self.model)
        return self._ema_state_dict()

    def load_state_dict(self, sd):
        """A dict without `ema` (an optimizer's, written without `ema_decay`) re-seeds the average from the current parameters, count 0."""
        self._refuse_in_scope("load_state_dict()")
        _order_behind_tail(self.model)
        self._ema_load(sd)
