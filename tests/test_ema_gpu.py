"""-m gpu: the exponential moving average of the trainable bucket (csrc/optim_ema.hip, optim.FusedAdamW(ema_decay=), optim.ModelEMA).

* owl_ema_update through the raw entry against the float64 recursion and its derived bound (tests/ema_reference.py), at the sizes where the grid changes
  shape; the degenerate decays bit for bit; nothing written past n;
* owl_adamw_step_ema: p / m / v / bf16 copy are the bits of owl_adamw_step_grouped (and of owl_adamw_step under a null table), the average the bits of
  owl_ema_update on the stepped parameters;
* the model level: the step is untouched by the average, ModelEMA gives the fused path's bits, the eval scope, the deferred tail, other trainable sets,
  the state round trip and two data-parallel ranks.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops, synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW, ModelEMA, ema_coefficients  # noqa: E402
from tests import ema_reference as R  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = 2048 * 256 * 4             # elements one trip of the capped grid covers
# one float4; two workgroups, the second ragged; a second grid-stride trip for the first 257 threads only
SIZES = [4, 1028, SWEEP + 1028]
# segment ends: an end at 8 (the smallest tensor slot), and for the largest size a segment [SWEEP / 2, SWEEP + 512) that straddles the trip boundary
SEG_ENDS = {4: [4], 1028: [8, 1028], SWEEP + 1028: [8, SWEEP // 2, SWEEP + 512, SWEEP + 1028]}
HEADS = ("box", "post_layernorm", "class_predictor", "queries")
EVERYTHING = ("backbone", "post_post_layernorm", "class_predictor", "box_head", "queries")
PAD, SENTINEL = 8, 123.0


def _rand(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _padded(x):
    """x followed by PAD sentinel elements, and the view of the first len(x)."""
    buf = torch.full((x.numel() + PAD,), SENTINEL, device=DEV)
    buf[: x.numel()] = x
    return buf, buf[: x.numel()]


# ---- owl_ema_update through the raw entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_raw_entry_inside_the_float64_bound(n):
    seed = _rand(n, 1)
    params = [_rand(n, 2 + k) for k in range(3)]
    d, w = R.decays(3, 0.9, True)              # 2/11, 3/12, 4/13: every step another pair
    buf, ema = _padded(seed)
    for p, dt, wt in zip(params, d, w):
        _lib.call("owl_ema_update", ops.stream(), ema, p, n, float(dt), float(wt))
    torch.cuda.synchronize()
    E, B = R.recursion(seed.cpu().numpy(), [p.cpu().numpy() for p in params], d, w)
    f = R.miss_factor(ema.cpu().numpy(), E, B)
    print(f"n={n}: max |ema - E| / B = {f:.3f}")
    assert f <= 1.0
    assert bool((buf[n:] == SENTINEL).all())


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_degenerate_decays_bit_for_bit(n):
    seed, p = _rand(n, 5), _rand(n, 6, scale=3.0)
    buf, ema = _padded(seed)
    _lib.call("owl_ema_update", ops.stream(), ema, p, n, *ema_coefficients(1.0))
    assert torch.equal(ema, seed)                          # d = 1, w = 0: unchanged
    _lib.call("owl_ema_update", ops.stream(), ema, p, n, *ema_coefficients(0.0))
    assert torch.equal(ema, p)                             # d = 0, w = 1: the parameters
    assert bool((buf[n:] == SENTINEL).all())


# ---- owl_adamw_step_ema through the raw entry --------------------------------------------------------------------------------------------------------
def _step_inputs(n):
    return dict(p=_rand(n, 10), g=_rand(n, 11), m=_rand(n, 12, 0.1), v=_rand(n, 13, 0.1).square(), ema=_rand(n, 14))


HYPER = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, step=3, grad_scale=0.5)


def _run_step(entry, n, x, table, max_norm=0.0, ema_dw=None):
    """One launch of `entry` on padded clones of x -> dict of the padded buffers (+ norm)."""
    bufs = {k: _padded(x[k]) for k in ("p", "m", "v", "ema")}
    bf_buf = torch.full((n + PAD,), SENTINEL, device=DEV, dtype=torch.bfloat16)
    norm = torch.zeros((), device=DEV)
    ws = None
    if max_norm > 0:
        nbytes = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_grad_norm_workspace_bytes", n, nbytes)
        ws = torch.zeros(int(nbytes.item()) // 8, dtype=torch.float64, device=DEV)
        _lib.call("owl_grad_sumsq", ops.stream(), x["g"], n, ws)
    h = HYPER
    head = (ops.stream(), bufs["p"][1], x["g"], bufs["m"][1], bufs["v"][1], bf_buf, n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], h["grad_scale"])
    if entry == "owl_adamw_step":
        _lib.call(entry, *head)
    else:
        if table is None:
            seg = (None, None, None, 0)
        else:
            ends = torch.tensor(table, dtype=torch.int64)
            seg = (ends, torch.tensor([h["lr"] * (1 + s) for s in range(len(table))]), torch.tensor([h["wd"] * (s % 2) for s in range(len(table))]), len(table))
        tail = (max_norm, ws, norm if max_norm > 0 else None)
        if entry == "owl_adamw_step_ema":
            _lib.call(entry, *head, *seg, *tail, bufs["ema"][1], *ema_dw)
        else:
            _lib.call(entry, *head, *seg, *tail)
    torch.cuda.synchronize()
    return dict({k: b[0] for k, b in bufs.items()}, bf16=bf_buf, norm=norm)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_step_ema_raw_entry_is_the_grouped_step_plus_the_update(n, clip):
    x = _step_inputs(n)
    dw = ema_coefficients(0.9)
    max_norm = 0.0
    if clip:
        max_norm = 0.5 * HYPER["grad_scale"] * float(torch.sqrt((x["g"].double() ** 2).sum()))          # half the scaled norm: the clip bites
    want = _run_step("owl_adamw_step_grouped", n, x, SEG_ENDS[n], max_norm)
    got = _run_step("owl_adamw_step_ema", n, x, SEG_ENDS[n], max_norm, dw)
    for k in ("p", "m", "v", "bf16", "norm"):
        assert torch.equal(got[k], want[k]), k             # (the padded buffers: the sentinels past n included)
    assert not torch.equal(got["p"][:n], x["p"])
    if clip:
        assert float(got["norm"]) > max_norm
    ema = x["ema"].clone()
    _lib.call("owl_ema_update", ops.stream(), ema, want["p"][:n], n, *dw)
    assert torch.equal(got["ema"][:n], ema)
    assert bool((got["ema"][n:] == SENTINEL).all()) and torch.equal(want["ema"][:n], x["ema"])


@pytest.mark.parametrize("n", SIZES)
def test_step_ema_null_table_is_the_one_group_step(n):
    x = _step_inputs(n)
    dw = ema_coefficients(2 / 11)
    want = _run_step("owl_adamw_step", n, x, None)
    got = _run_step("owl_adamw_step_ema", n, x, None, 0.0, dw)
    for k in ("p", "m", "v", "bf16"):
        assert torch.equal(got[k], want[k]), k
    ema = x["ema"].clone()
    _lib.call("owl_ema_update", ops.stream(), ema, want["p"][:n], n, *dw)
    assert torch.equal(got["ema"][:n], ema) and bool((got["ema"][n:] == SENTINEL).all())


# ---- the model level ---------------------------------------------------------------------------------------------------------------------------------
def _model(trainable=None, state=None):
    cfg = get_config("tiny")
    return cfg, OwlViT(cfg, weights.make_weights(cfg) if state is None else state, DEV, trainable=trainable)


def _bucket_grads(model, steps, seed=0):
    """Seeded random gradients over the tensors of the bucket; the alignment padding between tensors stays zero, as in training."""
    mask = torch.zeros(model.flat_numel)
    for n, o in model.flat_offsets.items():
        mask[o: o + model.p(n).numel()] = 1
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.randn(model.flat_numel, generator=g) * mask).to(DEV) for _ in range(steps)]


def _no_decay(model):
    return [n for n in model.flat_offsets if n.endswith(".bias") or "layer_norm" in n or "layernorm" in n or n == "queries"]


def _feed(opt, model, g):
    opt.zero_grad()
    model.flat_grad.copy_(g)
    opt.step()


def _batch(cfg, B=2):
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, max_boxes=4)
    return img, [torch.from_numpy(x).to(DEV) for x in labels], [torch.from_numpy(x).to(DEV) for x in boxes]


def _train_step(model, opt, crit, batch, **kw):
    img, lab, box = batch
    opt.zero_grad()
    pb, _, ps, _ = model(img, **kw)
    l = crit(ps, lab, pb, box)
    (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
    opt.step()


def _eval(model, img, **kw):
    with torch.no_grad():
        pb, _, ps, _ = model(img, **kw)
    return pb.clone(), ps.clone()


def _averaged_state(cfg, opt):
    """The numpy state a twin model is built from: the initial weights with the trainable tensors replaced by the average."""
    state = dict(weights.make_weights(cfg))
    for n, v in opt.ema_named().items():
        state[n] = v.detach().cpu().numpy()
    return state


@pytest.mark.parametrize("variant", ["one_group", "groups_and_clip", "heads_only", "full_fine_tune"])
def test_average_leaves_the_step_alone_and_stays_inside_the_bound(variant):
    trainable = {"heads_only": HEADS, "full_fine_tune": EVERYTHING}.get(variant)
    steps, decay = 3, 0.9

    def make(model, **kw):
        if variant == "groups_and_clip":
            kw.update(param_groups=[dict(params=_no_decay(model), lr=1.5e-3, weight_decay=0.0)], max_norm=50.0)
        return FusedAdamW(model, lr=3e-3, weight_decay=0.1, **kw)

    (_, model), (_, twin) = _model(trainable), _model(trainable)
    opt, plain = make(model, ema_decay=decay), make(twin)
    assert plain.ema is None and opt.ema.shape == model.flat_param.shape and opt.ema.dtype == torch.float32
    seed = model.flat_param.detach().clone()
    assert torch.equal(opt.ema, seed)
    seq = []
    for g in _bucket_grads(model, steps, seed=7):
        _feed(opt, model, g)
        _feed(plain, twin, g)
        seq.append(model.flat_param.detach().clone())
    torch.cuda.synchronize()
    for a, b, what in ((model.flat_param, twin.flat_param, "parameters"), (opt.exp_avg, plain.exp_avg, "exp_avg"), (opt.exp_avg_sq, plain.exp_avg_sq, "exp_avg_sq"),
                       (model.flat_bf16, twin.flat_bf16, "bf16 copy")):
        assert torch.equal(a, b), what
    if variant == "groups_and_clip":
        assert torch.equal(opt.last_grad_norm, plain.last_grad_norm) and float(opt.last_grad_norm) > 50.0
    assert opt.ema_updates == steps and plain.ema_updates == 0
    d, w = R.decays(steps, decay, True)
    E, B = R.recursion(seed.cpu().numpy(), [p.cpu().numpy() for p in seq], d, w)
    f = R.miss_factor(opt.ema.cpu().numpy(), E, B)
    print(f"{variant}: {model.flat_numel} elements, max |ema - E| / B = {f:.3f}")
    assert f <= 1.0
    assert not torch.equal(opt.ema, model.flat_param)


def test_model_ema_around_torch_adamw_gives_the_fused_bits():
    (_, model), (_, other) = _model(), _model()
    opt = FusedAdamW(model, lr=3e-3, weight_decay=0.1, ema_decay=0.9)
    topt = torch.optim.AdamW(other.parameters(), lr=3e-3, weight_decay=0.1)
    ema = ModelEMA(other, 0.9)
    for g in _bucket_grads(model, 3, seed=9):
        _feed(opt, model, g)
        for n, o in other.flat_offsets.items():
            other.p(n).grad = g[o: o + other.p(n).numel()].view(other.p(n).shape).clone()
        topt.step()
        np.testing.assert_allclose(other.flat_param.cpu().numpy(), model.flat_param.cpu().numpy(), rtol=1e-5, atol=1e-6)    # torch's step: close, not the same bits
        with torch.no_grad():
            other.flat_param.copy_(model.flat_param)           # fed the same parameters ...
        ema.update()
    assert ema.ema_updates == opt.ema_updates == 3
    assert torch.equal(ema.ema, opt.ema)                        # ... the same average, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(ema.ema_named().values(), opt.ema_named().values()))


# ---- the eval scope ----------------------------------------------------------------------------------------------------------------------------------
def test_scope_evaluates_the_average_and_training_continues_as_if_never_entered():
    def run(enter):
        cfg, model = _model()
        opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, ema_decay=0.9)
        crit, batch = PushPullLoss(cfg.n_classes, None), _batch(cfg)
        out = None
        for k in range(3):
            if k == 2 and enter:
                raw = _eval(model, batch[0])
                with opt.ema_weights():
                    out = _eval(model, batch[0])
                    sd = {n: v.clone() for n, v in model.state_dict().items()}
                    for call in (opt.step, opt.zero_grad, lambda: opt.load_state_dict(opt.state_dict())):
                        with pytest.raises(RuntimeError, match="inside"):
                            call()
                    with pytest.raises(RuntimeError, match="nested"):
                        with opt.ema_weights():
                            pass
                for n, v in opt.ema_named().items():
                    assert torch.equal(sd[n], v), n                   # the export path saw the average
                again = _eval(model, batch[0])
                assert torch.equal(raw[0], again[0]) and torch.equal(raw[1], again[1]) and not torch.equal(raw[1], out[1])
                twin = OwlViT(cfg, _averaged_state(cfg, opt), DEV)
                want = _eval(twin, batch[0])
                assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
            _train_step(model, opt, crit, batch)
        torch.cuda.synchronize()
        return model.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.ema.clone()

    for a, b, what in zip(run(False), run(True), ("parameters", "exp_avg", "exp_avg_sq", "ema")):
        assert torch.equal(a, b), what
    with pytest.raises(ValueError, match="ema_decay=None"):
        with FusedAdamW(_model()[1], lr=1e-3).ema_weights():
            pass


def test_scope_keeps_the_prefix_cache():
    cfg, model = _model()
    cache = model.enable_prefix_cache()
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, ema_decay=0.9)
    crit, batch = PushPullLoss(cfg.n_classes, None), _batch(cfg)
    ids = [100, 101]
    for _ in range(2):
        _train_step(model, opt, crit, batch, image_ids=ids)
    before = cache.stats
    assert before["slots"] == 2
    with opt.ema_weights():
        got = _eval(model, batch[0], image_ids=ids)
        assert cache.stats["slots"] == 2
    after = cache.stats
    assert after["slots"] == before["slots"] and after["misses"] == before["misses"] and after["hits"] == before["hits"] + 2
    want = _eval(OwlViT(cfg, _averaged_state(cfg, opt), DEV), batch[0])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- the deferred tail -------------------------------------------------------------------------------------------------------------------------------
def test_average_on_the_deferred_tail_is_bitwise_the_inline_schedule():
    def train(overlap):
        cfg, model = _model()
        opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap, ema_decay=0.9)
        crit, batch = PushPullLoss(cfg.n_classes, None), _batch(cfg)
        assert model.overlap_tail == overlap
        for _ in range(3):
            _train_step(model, opt, crit, batch)
        with opt.ema_weights():                     # right after a deferred step: the scope orders itself behind the tail
            out = _eval(model, batch[0])
        model.finish()
        torch.cuda.synchronize()
        return model.flat_param.clone(), opt.ema.clone(), out[0], out[1]

    for a, b, what in zip(train(False), train(True), ("parameters", "ema", "pred_boxes in the scope", "pred_sims in the scope")):
        assert torch.equal(a, b), what


# ---- the state round trip ----------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_continues_bitwise_and_old_dicts_reseed():
    _, model = _model()
    grads = _bucket_grads(model, 3, seed=5)
    make = lambda **kw: FusedAdamW(model, lr=3e-3, weight_decay=0.1, **kw)
    opt = make(ema_decay=0.9)
    for g in grads[:2]:
        _feed(opt, model, g)
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    assert sd["ema_updates"] == 2 and sd["ema_decay"] == 0.9 and sd["ema_warmup"] is True
    p2 = model.flat_param.detach().clone()
    _feed(opt, model, grads[2])
    want = (model.flat_param.clone(), opt.exp_avg.clone(), opt.ema.clone())

    with torch.no_grad():
        model.flat_param.copy_(p2)
    fresh = make(ema_decay=0.5, ema_warmup=False)
    fresh.load_state_dict(sd)
    assert fresh.ema_updates == 2 and fresh.ema_decay == 0.9 and fresh.ema_warmup is True
    _feed(fresh, model, grads[2])
    for a, b, what in zip(want, (model.flat_param, fresh.exp_avg, fresh.ema), ("parameters", "exp_avg", "ema")):
        assert torch.equal(a, b), what

    old = {k: v for k, v in sd.items() if not k.startswith("ema")}          # a dict written without an average
    with torch.no_grad():
        model.flat_param.copy_(p2)
    legacy = make(ema_decay=0.9)
    with torch.no_grad():
        legacy.ema.zero_()
    legacy.load_state_dict(old)
    assert legacy.step_count == 2 and legacy.ema_updates == 0 and torch.equal(legacy.ema, p2)
    _feed(legacy, model, grads[2])
    assert torch.equal(model.flat_param, want[0])                           # the step itself resumes bitwise
    fresh_avg = p2.clone()
    _lib.call("owl_ema_update", ops.stream(), fresh_avg, model.flat_param, model.flat_numel, *ema_coefficients(2 / 11))
    assert torch.equal(legacy.ema, fresh_avg)                               # the average restarts: seeded with p2, first warm-up decay


# ---- data parallel -----------------------------------------------------------------------------------------------------------------------------------
_WORKER = r'''
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from owl_vit_object_detection_amd import ddp, synth, weights
from owl_vit_object_detection_amd.config import get_config
from owl_vit_object_detection_amd.losses import PushPullLoss
from owl_vit_object_detection_amd.models import OwlViT
from owl_vit_object_detection_amd.optim import FusedAdamW
rank, world, local = ddp.init_from_env("gloo")
dev = torch.device("cuda", 0)                     # both ranks on the one visible GPU
cfg = get_config("tiny")
model = OwlViT(cfg, weights.make_weights(cfg), dev)
if rank == 1:
    model.flat_param.add_(0.5)                    # another starting point on this rank: the broadcast from rank 0 undoes it
opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, ema_decay=0.9)     # ... but the average is seeded HERE, from the pre-broadcast weights
seeded = opt.ema.clone()
dp = ddp.DataParallel(model, opt)
per = 2
img = torch.from_numpy(synth.make_images(cfg, per, first=rank * per)).to(dev)
labels, boxes = synth.make_targets(cfg, per, first=rank * per, max_boxes=4)
lab, box = [torch.from_numpy(x).to(dev) for x in labels], [torch.from_numpy(x).to(dev) for x in boxes]
crit = PushPullLoss(cfg.n_classes, None)
out = dict(seeded=seeded.cpu().numpy(), reseeded=opt.ema.cpu().numpy(), start=model.flat_param.cpu().numpy())
for k in range(2):
    opt.zero_grad()
    pb, _, ps, _ = model(img)
    l = crit(ps, lab, pb, box)
    (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
    out[f"local{{k}}"] = model.flat_grad.cpu().numpy()
    dp.sync_and_step()
torch.cuda.synchronize()
out.update(ema=opt.ema.cpu().numpy(), param=model.flat_param.cpu().numpy(), updates=np.int64(opt.ema_updates))
np.savez(os.path.join({out!r}, f"rank{{rank}}.npz"), **out)
dist.barrier(); dist.destroy_process_group()
'''


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.timeout(600)
def test_two_gloo_ranks_on_one_gpu_hold_the_same_average(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "OWL_FORCE_DIST"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), str(script)], capture_output=True, text=True, env=env, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert not np.array_equal(r0["seeded"], r1["seeded"])                    # rank 1 seeded its average before the broadcast ...
    np.testing.assert_array_equal(r0["reseeded"], r1["reseeded"])            # ... and DataParallel started it again from rank 0's weights
    np.testing.assert_array_equal(r0["reseeded"], r0["start"])
    assert int(r0["updates"]) == int(r1["updates"]) == 2
    assert r0["ema"].tobytes() == r1["ema"].tobytes() and r0["param"].tobytes() == r1["param"].tobytes()
    # one process, the summed gradients of the two ranks, the same grad_scale
    cfg, model = _model()
    np.testing.assert_array_equal(model.flat_param.cpu().numpy(), r0["start"])
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, ema_decay=0.9)
    opt.grad_scale = 0.5
    for k in range(2):
        _feed(opt, model, torch.from_numpy(r0[f"local{k}"] + r1[f"local{k}"]).to(DEV))
    assert model.flat_param.cpu().numpy().tobytes() == r0["param"].tobytes()
    assert opt.ema.cpu().numpy().tobytes() == r0["ema"].tobytes()
