"""-m gpu: the fused AdamW step against the float64 reference and its derived bounds (tests/adamw_reference.py).

* the raw entries owl_adamw_step, owl_adamw_step_grouped (clip off, and a clip that bites) and owl_adamw_step_ema (its p / m / v) on padded buffers:
  p', m' and v' inside their element-wise bounds on every input profile, at the reference run's learning rate among others, at steps 1, 2 and 1000, with
  segment tables whose ends are multiples of 4 but not of 8, and past one grid-stride trip under the full 32-row table; the bf16 copy is the RNE
  conversion of the kernel's own f32 p'; nothing is written past n; lr = 0 keeps p's bits;
* a three-step trajectory per entry, each step judged from the kernel's previous outputs;
* FusedAdamW on the tiny model for 12 steps with two groups, a clip that bites on some steps only, an LR scheduler and grad_scale 0.5, with and without
  the deferred tail: flat_param, exp_avg and exp_avg_sq at every step.

The bitwise agreement of the three entries is tests/test_ema_gpu.py's; the comparison with torch.optim.AdamW stays in tests/test_optim_gpu.py and
tests/test_optim_groups_gpu.py.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW, ema_coefficients  # noqa: E402
from tests import adamw_reference as R  # noqa: E402

DEV = "cuda"
SWEEP = 2048 * 256 * 4             # elements one trip of the capped grid covers
BIG = SWEEP + 1028
PAD, SENTINEL = 8, 123.0
# name -> lr, wd, beta1, beta2, eps
HYPERS = {"run": (3e-6, 0.1, 0.9, 0.999, 1e-8), "lr3e-3": (3e-3, 0.1, 0.9, 0.999, 1e-8), "b8_9": (1e-3, 0.0, 0.8, 0.9, 1e-6),
          "lr0": (0.0, 0.1, 0.9, 0.999, 1e-8)}
STEPS = (1, 2, 1000)
# ends that are multiples of 4 but not of 8, 4-element segments; the full 32 rows: 28 ends inside the first 128 elements, then a segment that straddles
# the trip boundary, so that a thread's second trip walks over 29 rows at once
SEG_ENDS = {4: [4], 1028: [4, 12, 16, 24, 512, 516, 1028],
            BIG: [4 * k for k in range(1, 29)] + [SWEEP // 2, SWEEP + 512, SWEEP + 516, SWEEP + 1028]}
ENTRIES = ("step", "grouped", "grouped_clip", "ema")
assert len(SEG_ENDS[BIG]) == 32


def _table(n, lr, wd):
    """Every row its own lr, 15 % apart; wd alternates between 0 and a non-zero value.  -> (ends, lr [rows] f32, wd [rows] f32)"""
    ends = SEG_ENDS[n]
    seg_lr = np.array([lr * 1.15 ** s for s in range(len(ends))], dtype=np.float32)
    seg_wd = np.array([(wd or 0.05) * (s % 2) for s in range(len(ends))], dtype=np.float32)
    return ends, seg_lr, seg_wd


def _padded(x, dtype=torch.float32):
    buf = torch.full((x.shape[0] + PAD,), SENTINEL, device=DEV, dtype=dtype)
    buf[: x.shape[0]] = torch.from_numpy(x).to(DEV)
    return buf


class _State:
    """Padded device buffers of one bucket; `launch` runs one entry on them and returns the reference's keyword arguments for that launch."""

    def __init__(self, p, m, v, null_bf16=False):
        self.n = p.shape[0]
        self.p, self.m, self.v = _padded(p), _padded(m), _padded(v)
        self.ema = _padded(p)
        self.bf16 = None if null_bf16 else torch.full((self.n + PAD,), SENTINEL, device=DEV, dtype=torch.bfloat16)

    def launch(self, entry, g, hyper, step, gs):
        n = self.n
        lr, wd, b1, b2, eps = HYPERS[hyper]
        gd = torch.from_numpy(g).to(DEV)
        head = (ops.stream(), self.p, gd, self.m, self.v, self.bf16, n, lr, b1, b2, eps, wd, step, gs)
        kw = dict(beta1=b1, beta2=b2, eps=eps, grad_scale=gs, step=step)
        if entry == "step":
            _lib.call("owl_adamw_step", *head)
            torch.cuda.synchronize()
            return dict(kw, lr=np.float32(lr), wd=np.float32(wd))
        ends, seg_lr, seg_wd = _table(n, lr, wd)
        max_norm, ws, norm = 0.0, None, None
        if entry != "grouped":          # a clip that bites: half the scaled norm (a zero gradient: any coefficient below 1)
            norm64 = math.sqrt(float(np.sum(g.astype(np.float64) ** 2))) * abs(gs)
            max_norm = R.f32(0.5 * norm64) if norm64 > 0 else 1e-7
            nbytes = torch.zeros(1, dtype=torch.int64)
            _lib.call("owl_grad_norm_workspace_bytes", n, nbytes)
            ws = torch.zeros(int(nbytes.item()) // 8, dtype=torch.float64, device=DEV)
            norm = torch.zeros((), device=DEV)
            _lib.call("owl_grad_sumsq", ops.stream(), gd, n, ws)
        tail = (torch.tensor(ends, dtype=torch.int64), torch.from_numpy(seg_lr), torch.from_numpy(seg_wd), len(ends), max_norm, ws, norm)
        if entry == "ema":
            _lib.call("owl_adamw_step_ema", *head, *tail, self.ema, *ema_coefficients(0.9))
        else:
            _lib.call("owl_adamw_step_grouped", *head, *tail)
        torch.cuda.synchronize()
        coef, rel = R.clip_coef(g, gs, max_norm)
        if max_norm > 0:
            assert coef < 0.6
        return dict(kw, lr=R.rows(ends, seg_lr, n), wd=R.rows(ends, seg_wd, n), coef=1.0 if coef is None else coef, coef_rel=rel)

    def outputs(self):
        n = self.n
        return tuple(x[:n].cpu().numpy() for x in (self.p, self.m, self.v))

    def check_layout(self):
        """Nothing past n; the bf16 copy is the RNE conversion of the kernel's own f32 p', bit for bit."""
        n = self.n
        for name in ("p", "m", "v"):
            assert bool((getattr(self, name)[n:] == SENTINEL).all()), name
        if self.bf16 is not None:
            assert bool((self.bf16[n:] == SENTINEL).all())
            assert torch.equal(self.bf16[:n].view(torch.int16), self.p[:n].bfloat16().view(torch.int16))


def _one_step(entry, n, profile, hyper, step, gs, null_bf16=False):
    """One launch on a fresh profile -> the miss factors of p', m', v'."""
    p, g, m, v = R.profile(profile, n, seed=step, beta1=HYPERS[hyper][2], scale=gs)
    st = _State(p, m, v, null_bf16)
    kw = st.launch(entry, g, hyper, step, gs)
    st.check_layout()
    got = st.outputs()
    if HYPERS[hyper][0] == 0.0:          # lr = 0: p keeps its bits while m and v still move
        assert got[0].tobytes() == p.tobytes()
        assert not np.array_equal(got[1], m)
        if profile != "tiny":            # (there g^2 underflows and b2 v may round back to a subnormal v: v' = v is right)
            assert not np.array_equal(got[2], v)
    return R.miss_factors(*got, R.step_reference(p, g, m, v, **kw))


@pytest.mark.parametrize("n", [4, 1028])
@pytest.mark.parametrize("entry", ENTRIES)
def test_raw_entry_inside_the_bounds_on_every_profile(entry, n):
    worst, outside = {}, []
    for pi, profile in enumerate(R.PROFILES):
        for hi, hyper in enumerate(HYPERS):
            for si, step in enumerate(STEPS):
                gs = (1.0, -0.5)[(pi + hi + si) % 2]
                f = _one_step(entry, n, profile, hyper, step, gs)
                for k, val in f.items():
                    if not val <= 1.0:          # (a NaN too)
                        outside.append((k, val, profile, hyper, step, gs))
                    if val > worst.get(k, (-1.0,))[0]:
                        worst[k] = (val, profile, hyper, step, gs)
    for k, (val, *where) in worst.items():
        print(f"{entry} n={n}: largest miss factor of {k}' {val:.3f} at {where}")
    assert not outside, outside


@pytest.mark.parametrize("profile,gs", [("unit", 1.0), ("eps_band", -0.5)])
@pytest.mark.parametrize("entry", ENTRIES)
def test_raw_entry_inside_the_bounds_past_one_trip(entry, profile, gs):
    f = _one_step(entry, BIG, profile, "run", 2, gs)
    print(f"{entry} n={BIG} {profile}: miss factors " + " ".join(f"{k}' {val:.3f}" for k, val in f.items()))
    assert max(f.values()) <= 1.0, f


@pytest.mark.parametrize("entry", ENTRIES)
def test_raw_entry_null_bf16_copy(entry):
    f = _one_step(entry, 1028, "unit", "lr3e-3", 3, 1.0, null_bf16=True)
    assert max(f.values()) <= 1.0, f


@pytest.mark.parametrize("entry", ENTRIES)
def test_raw_entry_three_step_trajectory(entry):
    n = 1028
    p, _, m, v = R.profile("eps_band", n, seed=100)
    st = _State(p, m, v)
    for step in (1, 2, 3):
        g = R.profile("eps_band", n, seed=100 + step)[1]
        kw = st.launch(entry, g, "run", step, 0.5)
        st.check_layout()
        got = st.outputs()
        f = R.miss_factors(*got, R.step_reference(p, g, m, v, **kw))          # from the kernel's own previous outputs
        print(f"{entry} trajectory step {step}: miss factors " + " ".join(f"{k}' {val:.3f}" for k, val in f.items()))
        assert max(f.values()) <= 1.0, (step, f)
        p, m, v = got


# ---- the class on the tiny model ------------------------------------------------------------------------------------------------------------------------
def _no_decay(model):
    return [n for n in model.flat_offsets if n.endswith(".bias") or "layer_norm" in n or "layernorm" in n or n == "queries"]


def _scheduler(opt):
    """A warm-up into a decay: lr changes at every step."""
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    return SequentialLR(opt, [LinearLR(opt, start_factor=0.1, end_factor=1.0, total_iters=4), CosineAnnealingLR(opt, T_max=10)], milestones=[4])


@pytest.mark.parametrize("overlap", [False, True])
def test_class_level_twelve_steps_inside_the_bounds(overlap):
    steps, gs = 12, 0.5
    cfg = get_config("tiny")
    model = OwlViT(cfg, weights.make_weights(cfg), DEV)
    n, names = model.flat_numel, list(model.flat_offsets)
    nd = set(_no_decay(model))
    # the group of every element from the bucket's layout alone: a tensor's slot runs to the next tensor's offset
    group = np.zeros(n, dtype=np.int64)
    mask = np.zeros(n, dtype=bool)
    for k, name in enumerate(names):
        o = model.flat_offsets[name]
        end = model.flat_offsets[names[k + 1]] if k + 1 < len(names) else n
        group[o:end] = 1 if name in nd else 0
        mask[o: o + model.p(name).numel()] = True
    # an eps_band-like bucket, alignment padding zero; every other step four times as large, the clip between the two norms
    rng = np.random.default_rng(12)
    grads = []
    for k in range(steps):
        g = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-12.0, -4.0, n) * (4.0 if k % 2 else 1.0)
        grads.append((g * mask).astype(np.float32))
    norms = [math.sqrt(float(np.sum(g.astype(np.float64) ** 2))) * gs for g in grads]
    max_norm = 2.0 * min(norms)
    opt = FusedAdamW(model, lr=3e-6, weight_decay=0.1, overlap=overlap, max_norm=max_norm,
                     param_groups=[dict(params=sorted(nd, key=names.index), lr=1.5e-6, weight_decay=0.0)])
    opt.grad_scale = gs
    assert len(opt.param_groups) == 2 and model.overlap_tail == overlap
    sched = _scheduler(opt)

    def state():
        model.finish()
        torch.cuda.synchronize()
        return tuple(x.detach().cpu().numpy() for x in (model.flat_param, opt.exp_avg, opt.exp_avg_sq))

    p, m, v = state()
    worst, coefs, lrs = {}, [], []
    for k in range(steps):
        lr = np.array([g["lr"] for g in opt.param_groups], dtype=np.float32)          # rounded to f32 as the binding rounds them
        wd = np.array([g["weight_decay"] for g in opt.param_groups], dtype=np.float32)
        b1, b2 = opt.param_groups[0]["betas"]
        opt.zero_grad()
        model.flat_grad.copy_(torch.from_numpy(grads[k]).to(DEV))
        opt.step()
        sched.step()
        got = state()
        coef, rel = R.clip_coef(grads[k], gs, opt.max_norm)
        ref = R.step_reference(p, grads[k], m, v, lr=lr[group], wd=wd[group], beta1=b1, beta2=b2, eps=opt.param_groups[0]["eps"], grad_scale=gs,
                               step=k + 1, coef=coef, coef_rel=rel)
        f = R.miss_factors(*got, ref)
        print(f"overlap {overlap} step {k + 1}: lr {float(lr[0]):.3e} coef {coef:.3f} miss factors " + " ".join(f"{key} {val:.3f}" for key, val in f.items()))
        for key, val in f.items():
            worst[key] = max(worst.get(key, 0.0), val)
        assert max(f.values()) <= 1.0, (k + 1, f)
        assert torch.equal(model.flat_bf16.view(torch.int16), model.flat_param.detach().bfloat16().view(torch.int16))
        coefs.append(coef)
        lrs.append(float(lr[0]))
        p, m, v = got
    print(f"overlap {overlap}: largest miss factors " + " ".join(f"{key} {val:.3f}" for key, val in worst.items()))
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)              # the clip bit on some steps and not on others
    assert len(set(lrs)) == steps                                                    # another lr at every step
    sd = opt.state_dict()
    assert opt.step_count == steps == sd["step"] and sd["exp_avg"] is opt.exp_avg and sd["exp_avg_sq"] is opt.exp_avg_sq
