"""-m gpu: FusedAdamW with parameter groups, torch LR schedulers and fused gradient-norm clipping.

* owl_grad_sumsq through the raw entry against a float64 norm, at the sizes where the kernel changes path; run-to-run bits;
* the clipped, grouped step against torch.optim.AdamW with the same groups at the one-group kernel's own bound (tests/test_optim_gpu.py);
* neutrality: a clip that never bites / groups that do not differ give the bits of the one-group kernel;
* torch LR schedulers drive the launches; the deferred tail and the state round trip are bitwise.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops, synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402

DEV = "cuda"
RTOL, ATOL = 2e-6, 1e-7            # the project's bound for the AdamW kernel against torch (tests/test_optim_gpu.py)
F32_ROUND = 2.0 ** -23             # one f32 rounding of an f64 result whose own error (about n * 2^-53) is far below it


def _model():
    cfg = get_config("tiny")
    return cfg, OwlViT(cfg, weights.make_weights(cfg), DEV)


def _no_decay(model):
    """LayerNorm affines, biases and the query bank."""
    return [n for n in model.flat_offsets if n.endswith(".bias") or "layer_norm" in n or "layernorm" in n or n == "queries"]


def _bucket_grads(model, steps, seed=0):
    """Seeded random gradients over the tensors of the bucket; the alignment padding between tensors stays zero, as in training."""
    mask = torch.zeros(model.flat_numel)
    for n, o in model.flat_offsets.items():
        mask[o: o + model.p(n).numel()] = 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randn(model.flat_numel, generator=g) * mask).to(DEV) for _ in range(steps)]


def _norm64(g):
    return float(torch.sqrt((g.double() ** 2).sum()))


# ---- the reduction through the raw entry ---------------------------------------------------------------------------------------------------------
# A workgroup takes 256 float4; the grid is capped at 1024 workgroups, so one grid-stride trip covers 1024 * 256 * 4 = 1,048,576 elements and the kernel's
# unrolled body takes four trips at once.  8: one partly filled wave; 1032: two workgroups; + 8 past one trip: the smallest second trip;
# 2,097,152 + 8: one float4 past two trips (past ONE trip of a grid capped like the AdamW kernel's); 4,194,304 + 8: the unrolled body and the remainder loop.
SUMSQ_SIZES = [8, 1032, 1048576 + 8, 2097152 + 8, 4194304 + 8]


@pytest.mark.parametrize("kind", ["normal", "spike"])
@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_grad_norm_raw_entry_against_float64(n, kind):
    if kind == "normal":
        g = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
    else:
        g = torch.full((n,), 1e-4, device=DEV)
        g[n - 3] = 1e4                      # one large element among small ones, in the last float4
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_grad_norm_workspace_bytes", n, nbytes)
    assert int(nbytes.item()) == 8 * min((n // 4 + 255) // 256, 1024)
    ws = [torch.full((int(nbytes.item()) // 8,), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2)]
    for w in ws:
        _lib.call("owl_grad_sumsq", ops.stream(), g, n, w)
    assert torch.equal(ws[0].view(torch.int64), ws[1].view(torch.int64))          # two runs on one buffer: identical bits
    ref = _norm64(g)
    # the f32 norm the step reports: a step with lr = 0 and a clip that cannot bite, on scratch buffers
    p, m, v, norm = torch.ones(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros((), device=DEV)
    end, lr, wd = torch.tensor([n], dtype=torch.int64), torch.zeros(1), torch.zeros(1)
    for scale in (1.0, -0.5):
        _lib.call("owl_adamw_step_grouped", ops.stream(), p, g, m, v, None, n, 0.0, 0.9, 0.999, 1e-8, 0.0, 1, scale, end, lr, wd, 1, 1e30, ws[0], norm)
        got = float(norm)
        print(f"n={n} {kind} scale={scale}: norm f32 {got!r} f64 {ref * abs(scale)!r} rel err {abs(got - ref * abs(scale)) / (ref * abs(scale)):.3e}")
        assert abs(got - ref * abs(scale)) <= F32_ROUND * ref * abs(scale)
    assert float(p.min()) == 1.0 == float(p.max())                                # lr = 0, no decay: the parameters did not move
    got = float(torch.sqrt(ws[0].sum()).float())                                  # and the partial sums themselves
    assert abs(got - ref) <= F32_ROUND * ref


# ---- the clipped, grouped step against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clipped_grouped_step_matches_torch(grad_scale):
    cfg, model = _model()
    nd = _no_decay(model)
    lr, steps = 3e-3, 3
    grads = _bucket_grads(model, steps)
    norm1 = _norm64(grads[0]) * grad_scale
    max_norm = float(torch.tensor(0.5 * norm1, dtype=torch.float32))               # half of the first step's norm: the clip bites
    opt = FusedAdamW(model, lr=lr, weight_decay=0.1, param_groups=[dict(params=nd, lr=0.5 * lr, weight_decay=0.0)], max_norm=max_norm)
    opt.grad_scale = grad_scale
    assert len(opt.param_groups) == 2 and 2 < len(opt._segments) <= 32
    ref = {n: model.p(n).detach().clone().requires_grad_(True) for n in model.flat_offsets}
    topt = torch.optim.AdamW([dict(params=[ref[n] for n in ref if n not in nd], lr=lr, weight_decay=0.1),
                              dict(params=[ref[n] for n in nd], lr=0.5 * lr, weight_decay=0.0)])
    for k, g in enumerate(grads):
        opt.zero_grad()
        model.flat_grad.copy_(g)
        opt.step()
        norm = _norm64(g) * grad_scale
        coef = torch.tensor(min(1.0, max_norm / (norm + 1e-6)), dtype=torch.float64).float().to(DEV)       # float64, then rounded to f32
        assert float(coef) < 0.6
        scaled = g * grad_scale * coef
        for n, o in model.flat_offsets.items():
            ref[n].grad = scaled[o: o + ref[n].numel()].view(ref[n].shape).clone()
        topt.step()
        got = float(opt.last_grad_norm)
        print(f"step {k + 1} grad_scale {grad_scale}: last_grad_norm {got!r} f64 {norm!r} rel err {abs(got - norm) / norm:.3e}")
        assert abs(got - norm) <= F32_ROUND * norm
        for n in model.flat_offsets:
            np.testing.assert_allclose(model.p(n).detach().cpu().numpy(), ref[n].detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=n)
        assert torch.equal(model.flat_bf16, model.flat_param.bfloat16())


# ---- neutrality ---------------------------------------------------------------------------------------------------------------------------------------
def _two_steps(make_opt):
    cfg, model = _model()
    opt = make_opt(model)
    for g in _bucket_grads(model, 2, seed=3):
        opt.zero_grad()
        model.flat_grad.copy_(g)
        opt.step()
    torch.cuda.synchronize()
    return opt, (model.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), model.flat_bf16.clone())


@pytest.mark.parametrize("variant", ["clip_never_bites", "one_explicit_group", "two_equal_groups", "two_equal_groups_clip_never_bites"])
def test_neutral_settings_give_the_bits_of_the_one_group_kernel(variant):
    kw = dict(lr=3e-3, weight_decay=0.1)
    make = {
        "clip_never_bites": lambda m: FusedAdamW(m, **kw, max_norm=1e30),
        "one_explicit_group": lambda m: FusedAdamW(m, lr=1.0, weight_decay=0.0, param_groups=[dict(params=list(m.flat_offsets), **kw)]),
        "two_equal_groups": lambda m: FusedAdamW(m, **kw, param_groups=[dict(params=_no_decay(m), **kw)]),
        "two_equal_groups_clip_never_bites": lambda m: FusedAdamW(m, **kw, param_groups=[dict(params=_no_decay(m), **kw)], max_norm=1e30),
    }[variant]
    _, plain = _two_steps(lambda m: FusedAdamW(m, **kw))
    opt, got = _two_steps(make)
    assert len(opt.param_groups) == (2 if "two" in variant else 1)
    for a, b, what in zip(plain, got, ("parameters", "exp_avg", "exp_avg_sq", "bf16 copy")):
        assert torch.equal(a, b), what
    if opt.max_norm is not None:
        assert float(opt.last_grad_norm) > 100.0           # the norm is still reported (about sqrt(175,000) for unit normal gradients)


# ---- schedulers -------------------------------------------------------------------------------------------------------------------------------------
def _scheduler(opt):
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR, SequentialLR
    return SequentialLR(opt, [LinearLR(opt, start_factor=0.1, end_factor=1.0, total_iters=2), CosineAnnealingLR(opt, T_max=4)], milestones=[2])


def _batch(cfg, B=2):
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, max_boxes=4)
    return img, [torch.from_numpy(x).to(DEV) for x in labels], [torch.from_numpy(x).to(DEV) for x in boxes]


def _loss(crit, ps, lab, pb, box):
    l = crit(ps, lab, pb, box)
    return l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]


def test_sequential_lr_drives_every_launch():
    cfg, model = _model()
    img, lab, box = _batch(cfg)
    crit = PushPullLoss(cfg.n_classes, None)
    p0 = model.flat_param.detach().clone()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        opt = FusedAdamW(model, lr=3e-4, weight_decay=0.1)
        sched = _scheduler(opt)
        vals, grads, params, lrs = [], [], [], []
        for it in range(6):
            opt.zero_grad()
            pb, _, ps, _ = model(img)
            loss = _loss(crit, ps, lab, pb, box)
            loss.backward()
            grads.append(model.flat_grad.clone())
            lrs.append(sched.get_last_lr()[0])
            assert opt.lr == lrs[-1]
            opt.step()
            sched.step()
            params.append(model.flat_param.detach().clone())
            vals.append(float(loss))
    assert not [str(w.message) for w in caught if "lr_scheduler" in str(w.message) or "optimizer.step" in str(w.message)]
    assert vals[-1] < vals[0], vals                             # the loss goes down on a fixed batch
    assert lrs[0] == pytest.approx(3e-5) and lrs[2] == pytest.approx(3e-4) and lrs[5] < lrs[4] < lrs[3] < lrs[2]      # warm-up, then the cosine
    # the lr each launch used: the same six steps through torch.optim.AdamW + the same scheduler on a clone of the bucket, with the recorded gradients
    ref = p0.clone().requires_grad_(True)
    topt = torch.optim.AdamW([ref], lr=3e-4, weight_decay=0.1)
    tsched = _scheduler(topt)
    for it in range(6):
        assert tsched.get_last_lr()[0] == lrs[it]
        ref.grad = grads[it].clone()
        topt.step()
        tsched.step()
        np.testing.assert_allclose(params[it].cpu().numpy(), ref.detach().cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg=f"step {it + 1}")


# ---- the deferred tail ------------------------------------------------------------------------------------------------------------------------------
def test_clipped_grouped_step_on_the_deferred_tail_is_bitwise_the_inline_schedule():
    def train(overlap, steps=2):
        cfg, model = _model()
        img, lab, box = _batch(cfg)
        crit = PushPullLoss(cfg.n_classes, None)
        opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap, max_norm=0.05,
                         param_groups=[dict(params=_no_decay(model), lr=5e-4, weight_decay=0.0)])
        assert model.overlap_tail == overlap
        for s in range(steps):
            opt.zero_grad()
            pb, _, ps, _ = model(img)
            _loss(crit, ps, lab, pb, box).backward()
            opt.step()
        model.finish()
        torch.cuda.synchronize()
        return model.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.last_grad_norm.cpu()

    p0, m0, v0, n0 = train(False)
    p1, m1, v1, n1 = train(True)
    print(f"gradient norm of the second step: {float(n0)!r}")
    assert float(n0) > 0.05, n0                                  # the clip bit
    assert torch.equal(n0, n1) and torch.equal(m0, m1) and torch.equal(v0, v1) and torch.equal(p0, p1)


# ---- the state round trip ---------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_after_scheduled_clipped_steps():
    cfg, model = _model()
    grads = _bucket_grads(model, 3, seed=5)

    def make():
        return FusedAdamW(model, lr=3e-3, weight_decay=0.1, max_norm=100.0, param_groups=[dict(params=_no_decay(model), lr=1.5e-3, weight_decay=0.0)])

    def one(opt, g):
        opt.zero_grad()
        model.flat_grad.copy_(g)
        opt.step()

    opt = make()
    sched = _scheduler(opt)
    for g in grads[:2]:
        one(opt, g)
        sched.step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    assert sd["step"] == 2 and sd["max_norm"] == 100.0 and [set(g) for g in sd["groups"]] == [{"lr", "weight_decay", "initial_lr"}] * 2
    assert sd["groups"][0]["lr"] == sched.get_last_lr()[0] == pytest.approx(3e-3) and sd["groups"][1]["initial_lr"] == 1.5e-3
    p2 = model.flat_param.detach().clone()
    one(opt, grads[2])
    want = (model.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.last_grad_norm.clone())

    with torch.no_grad():
        model.flat_param.copy_(p2)
    fresh = FusedAdamW(model, lr=1.0, weight_decay=0.5, max_norm=1.0, param_groups=[dict(params=_no_decay(model), lr=2.0, weight_decay=0.25)])
    fresh.load_state_dict(sd)
    assert fresh.step_count == 2 and fresh.max_norm == 100.0
    one(fresh, grads[2])
    got = (model.flat_param.clone(), fresh.exp_avg.clone(), fresh.exp_avg_sq.clone(), fresh.last_grad_norm.clone())
    for a, b, what in zip(want, got, ("parameters", "exp_avg", "exp_avg_sq", "last_grad_norm")):
        assert torch.equal(a, b), what

    old = {k: sd[k] for k in ("step", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay")}       # a dict written before the groups existed
    legacy = make()
    legacy.load_state_dict(old)
    assert legacy.step_count == 2 and torch.equal(legacy.exp_avg, sd["exp_avg"]) and [g["lr"] for g in legacy.param_groups] == [3e-3, 1.5e-3]
