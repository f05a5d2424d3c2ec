"""-m gpu: a model built at a rectangular input size -- `load_model(..., image_size=(H, W))` / `OwlViT(cfg)` with a rectangular config.

`tiny` (native 96, a 6 x 6 table) runs at (96, 160), (160, 96), (64, 128) and (64, 144) -- the last is 4 x 9, the 36 patches of the native table, which
must still be resampled --, `tiny-p14` of tests/test_trainable_sets_gpu.py (14-pixel patches) at (112, 70).  The recipe is
tests/test_resolution_gpu.py::_reference: the oracle's `model_forward` runs UNCHANGED on a state whose position table is the float64 reference's table
(tests/rect_reference.forward64_hw) cast to f32, with `O.box_bias` replaced for the call by rect_reference.box_bias_hw (the oracle's own is square); the
expected gradient of the native table is adjoint64_hw of the oracle's.  Bounds: tests/test_model_gpu.py's on the outputs, the project's gradient band
(rel-L2 < 2e-2, cosine > 0.9995)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import owl_oracle as O  # noqa: E402  (checker only)
from owl_vit_object_detection_amd import synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import OpenVocabLoss, PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.metrics import MeanAveragePrecision  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT, PostProcess, check_detect_args, load_model  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor, DevicePrefetcher, TrainAugment  # noqa: E402
from tests import rect_reference as RR  # noqa: E402
from tests import test_trainable_sets_gpu as TS  # noqa: E402  (its gradient measure, band and the tiny-p14 config)
from tests.golden.make_golden_open_vocab import D_BOXES, model_tolerance  # noqa: E402
from tests.test_model_gpu import TOL_BOXES, TOL_SIMS_SMALLCFG  # noqa: E402

DEV = "cuda"
POS = "backbone.embeddings.position_embedding.weight"
LABELMAP = {i: f"c{i}" for i in range(4)}
CASES = [("tiny", (96, 160)), ("tiny", (160, 96)), ("tiny", (64, 128)), ("tiny", (64, 144)), ("tiny-p14", (112, 70))]
IDS = [f"{c}-{h}x{w}" for c, (h, w) in CASES]
B = 2
LOSSES = ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")
_ref_cache = {}


class _OracleView:
    """The rectangular config as the oracle reads it: every field is the config's; `grid` -- which the oracle hands to `box_bias` alone, replaced for the
    call -- is None (OwlConfig.grid raises on a rectangle, by design)."""
    grid = None

    def __init__(self, cfg):
        self._cfg = cfg

    def __getattr__(self, k):
        return getattr(self._cfg, k)


def _rect_cfg(cname, hw):
    cfg0 = TS._cfg(cname)
    return cfg0, cfg0.replace(image_size=hw, pos_grid=cfg0.grid)


def _build(cname, hw, state, **kw):
    cfg0, cfg = _rect_cfg(cname, hw)
    if cname == "tiny":
        return load_model(LABELMAP, DEV, arch="tiny", state=state, image_size=hw, **kw)
    return OwlViT(cfg, state, DEV, **kw)


def _reference(cname, hw):
    if (cname, hw) in _ref_cache:
        return _ref_cache[(cname, hw)]
    cfg0, cfg = _rect_cfg(cname, hw)
    g0, gh, gw = cfg0.grid, cfg.grid_h, cfg.grid_w
    Wnp = weights.make_weights(cfg0)
    img = synth.make_images(cfg, B)
    assert img.shape == (B, 3) + tuple(hw)
    w = {k: torch.from_numpy(v) for k, v in Wnp.items()}
    w[POS] = RR.forward64_hw(w[POS], g0, gh, gw).float()
    gen = torch.Generator().manual_seed(5)
    d_boxes = torch.randn(B, cfg.patches, 4, generator=gen) * 0.1
    d_sims = torch.randn(B, cfg.patches, cfg.n_classes, generator=gen) * 0.1
    ww = {n: t.clone().requires_grad_(True) for n, t in w.items()}
    taps = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(O, "box_bias", lambda grid: RR.box_bias_hw(gh, gw).float())
        rb, rs = O.model_forward(_OracleView(cfg), ww, torch.from_numpy(img), taps)
    with torch.no_grad():          # near-tie prompt routes get no upstream (tests/test_resolution_gpu.py::_reference)
        e = torch.nn.functional.linear(taps["feats"], w["class_predictor.dense0.weight"], w["class_predictor.dense0.bias"])
        e = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
        q = w["queries"] / torch.linalg.norm(w["queries"], dim=-1, keepdim=True) + 1e-6
        top2 = (e @ q.transpose(1, 2)).view(B, cfg.patches, cfg.n_classes, 3).topk(2, dim=-1).values
        d_sims = d_sims * ((top2[..., 0] - top2[..., 1]) > 0.02).float()
    torch.autograd.backward([rb, rs], [d_boxes, d_sims])
    gref = {n: ww[n].grad.detach() for n in ww}
    gref[POS] = RR.adjoint64_hw(gref[POS], g0, gh, gw).float()
    out = dict(Wnp=Wnp, img=img, d_boxes=d_boxes, d_sims=d_sims, rb=rb.detach(), rs=rs.detach(), gref=gref, cfg=cfg, g0=g0, gh=gh, gw=gw)
    _ref_cache[(cname, hw)] = out
    return out


@pytest.mark.parametrize("cname,hw", CASES, ids=IDS)
def test_forward_matches_the_oracle(cname, hw):
    r = _reference(cname, hw)
    model = _build(cname, hw, r["Wnp"])
    cfg = model.cfg
    assert cfg.image_size == hw and (cfg.grid_h, cfg.grid_w, cfg.native_grid) == (r["gh"], r["gw"], r["g0"]) and not model._train_emb
    assert tuple(model.p(POS).shape) == (r["g0"] ** 2 + 1, cfg.hidden) and tuple(model._pos_used.shape) == (cfg.tokens, cfg.hidden)
    assert tuple(model.box_bias.shape) == (cfg.patches, 4)
    with torch.no_grad():
        pb, _, ps, _ = model(torch.from_numpy(r["img"]).to(DEV))
    assert pb.shape == (B, cfg.patches, 4) and ps.shape == (B, cfg.patches, cfg.n_classes)
    eb, es = float((pb.cpu() - r["rb"]).abs().max()), float((ps.cpu() - r["rs"]).abs().max())
    print(f"RECT {cname} at {hw} (T = {cfg.tokens}): max|d boxes|={eb:.3e} max|d sims|={es:.3e}")
    assert eb < TOL_BOXES and es < TOL_SIMS_SMALLCFG, (eb, es)


@pytest.mark.parametrize("keep", [TS.EVERYTHING, None], ids=["everything", "default"])
@pytest.mark.parametrize("cname,hw", CASES, ids=IDS)
def test_gradients_match_the_oracle(cname, hw, keep):
    r = _reference(cname, hw)
    model = _build(cname, hw, r["Wnp"], **({} if keep is None else dict(trainable=keep)))
    pb, _, ps, _ = model(torch.from_numpy(r["img"]).to(DEV))
    torch.autograd.backward([pb, ps], [r["d_boxes"].to(DEV), r["d_sims"].to(DEV)])
    model.finish()
    torch.cuda.synchronize()
    names = list(model.flat_offsets)
    if keep is not None:
        assert set(names) == set(weights.param_shapes(model.cfg))
    grads = {n: model.p(n).grad.detach().float().cpu() for n in names}
    tag = f"{'everything' if keep else 'default'} {cname} at {hw}"
    worst, worst_cos = TS._grad_report(grads, {n: r["gref"][n] for n in names}, tag)
    assert worst < TS.REL_L2 and worst_cos > TS.COS, (worst, worst_cos)
    if keep is not None:
        assert tuple(grads[POS].shape) == (r["g0"] ** 2 + 1, model.cfg.hidden)          # the native shape
        w, c = TS._grad_report({POS: grads[POS]}, {POS: r["gref"][POS]}, f"{tag}: {POS}")
        assert w < TS.REL_L2 and c > TS.COS, (w, c)


def _step(model, img, seed=0, finish=True):
    cfg = model.cfg
    labels, boxes = synth.make_targets(cfg, img.shape[0], max_boxes=5, seed=1234 + seed)
    model.flat_grad.zero_()
    pb, _, ps, _ = model(img)
    l = PushPullLoss(cfg.n_classes, None)(ps, [torch.from_numpy(x).to(DEV) for x in labels], pb, [torch.from_numpy(x).to(DEV) for x in boxes])
    sum(l[k] for k in LOSSES).backward()
    if finish:
        model.finish()
    torch.cuda.synchronize()
    return pb.detach().clone(), ps.detach().clone(), torch.stack([l[k].detach() for k in LOSSES]), model.flat_grad.clone()


def test_a_square_pair_is_bitwise_the_int():
    Wnp = weights.make_weights(get_config("tiny"))
    res = []
    for size in (128, (128, 128)):
        model = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=size, trainable=TS.EVERYTHING)
        assert model.cfg.image_size == 128 and model.cfg.grid == 8
        img = torch.from_numpy(synth.make_images(model.cfg, B)).to(DEV)
        res.append(_step(model, img))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][3].abs().max()) > 0
    native = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=(96, 96))
    assert native._pos_used is None and native.cfg == get_config("tiny").replace(n_classes=4)


def _train(model, steps, overlap, lr=1e-3):
    cfg = model.cfg
    labels, boxes = synth.make_targets(cfg, 4, max_boxes=5)
    lab = [torch.from_numpy(x).to(DEV) for x in labels]; box = [torch.from_numpy(x).to(DEV) for x in boxes]
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=lr, weight_decay=0.1, overlap=overlap)
    gen = torch.Generator(device="cpu").manual_seed(7)
    imgs = [torch.randn(4, 3, *cfg.image_hw, generator=gen).to(DEV) for _ in range(steps)]
    hist = []
    for s in range(steps):
        opt.zero_grad()
        pb, _, ps, _ = model(imgs[s])
        l = crit(ps, lab, pb, box)
        loss = sum(l[k] for k in LOSSES)
        loss.backward()
        hist.append(loss.detach())
        opt.step()
    model.finish()
    torch.cuda.synchronize()
    return opt, torch.stack(hist).cpu()


def test_deferred_tail_is_bitwise_the_inline_schedule_over_three_steps():
    out = []
    for overlap in (False, True):
        model = load_model(LABELMAP, DEV, arch="tiny", state=weights.make_weights(get_config("tiny")), image_size=(96, 160), trainable=TS.EVERYTHING)
        p0 = model.flat_param.clone()
        _, hist = _train(model, 3, overlap=overlap)
        assert model.overlap_tail == overlap and not torch.equal(p0, model.flat_param)
        out.append((hist, model.flat_param.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and bool(torch.isfinite(out[0][0]).all())


def test_state_written_at_a_rectangle_loads_at_the_square_and_the_other_rectangle():
    Wnp = weights.make_weights(get_config("tiny"))
    m = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=(96, 160), trainable=TS.EVERYTHING)
    opt_r, _ = _train(m, 1, overlap=False)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    assert tuple(sd[POS].shape) == (37, 128)
    for size in (96, (160, 96)):
        other = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=size, trainable=TS.EVERYTHING)
        assert list(other.flat_offsets.items()) == list(m.flat_offsets.items()) and other.flat_numel == m.flat_numel
        opt = FusedAdamW(other, lr=1e-3, weight_decay=0.1)
        opt.load_state_dict(opt_r.state_dict())
        assert opt.step_count == 1 and torch.equal(opt.exp_avg, opt_r.exp_avg)
        other.load_state_dict(m.state_dict())
        assert torch.equal(other.flat_param, m.flat_param)
        fresh = load_model(LABELMAP, DEV, arch="tiny", state=sd, image_size=size, trainable=TS.EVERYTHING)
        img = torch.from_numpy(synth.make_images(other.cfg, B)).to(DEV)
        with torch.no_grad():
            a, b = other(img), fresh(img)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])          # (the used table was re-made from the loaded parameter)


def test_prefix_cache_cold_and_warm_is_bitwise_the_model_without_it():
    Wnp = weights.make_weights(get_config("tiny"))
    model = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=(96, 160))
    twin = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=(96, 160))
    model.enable_prefix_cache()
    pool = torch.from_numpy(synth.make_images(model.cfg, 5)).to(DEV)
    labels, boxes = synth.make_targets(model.cfg, 5, max_boxes=5)
    lab = [torch.from_numpy(x).to(DEV) for x in labels]; box = [torch.from_numpy(x).to(DEV) for x in boxes]

    def step(m, idx, ids):
        m.finish()
        m.flat_grad.zero_()
        pb, _, ps, _ = m(pool[idx], **(dict(image_ids=[900 + i for i in idx]) if ids else {}))
        l = PushPullLoss(m.cfg.n_classes, None)(ps, [lab[i] for i in idx], pb, [box[i] for i in idx])
        sum(l[k] for k in LOSSES).backward()
        m.finish()
        torch.cuda.synchronize()
        return pb.detach().clone(), ps.detach().clone(), torch.stack([l[k].detach() for k in LOSSES]), m.flat_grad.clone()

    for tag, idx in (("cold", [0, 1, 2, 3]), ("warm", [3, 0, 2, 1]), ("mixed", [4, 1])):
        for x, y in zip(step(model, idx, True), step(twin, idx, False)):
            assert torch.equal(x, y), tag
    s = model.prefix_cache.stats
    assert s["hits"] == 5 and s["misses"] == 5


@pytest.mark.parametrize("cname,hw", [CASES[0], CASES[3], CASES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_every_image_of_a_batch_carries_the_bits_of_its_batch_of_one(cname, hw):
    r = _reference(cname, hw)
    model = _build(cname, hw, r["Wnp"])
    img = torch.from_numpy(synth.make_images(model.cfg, 3)).to(DEV)
    with torch.no_grad():
        pb, _, ps, _ = model(img)
        pb, ps = pb.clone(), ps.clone()
        for b in range(3):
            ob, _, os_, _ = model(img[b:b + 1])
            assert torch.equal(ob[0], pb[b]) and torch.equal(os_[0], ps[b]), b


# ---- HF ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def f18(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f18_rect.npz")))


def _fixture_pixels(g):
    x = g["pixel_levels"].astype(np.float64) / 255.0
    return ((x - synth.CLIP_MEAN[:, None, None]) / synth.CLIP_STD[:, None, None]).astype(np.float32)


def test_detect_at_96x160_against_hf(f18):
    g = f18
    hw = tuple(int(v) for v in g["hw"])
    head = {k: g["head/" + k] for k in weights.LOGIT_HEAD_KEYS}
    model = load_model(LABELMAP, DEV, arch="tiny", state=weights.make_weights(get_config("tiny")), image_size=hw, logit_head=head)
    img = torch.from_numpy(_fixture_pixels(g)).to(DEV)
    assert tuple(img.shape[2:]) == hw == (96, 160)
    boxes, logits = model.detect(img, torch.from_numpy(g["query_embeds"]), torch.from_numpy(g["query_mask"]))
    torch.cuda.synchronize()
    ref = g["logits"].astype(np.float64)
    Bf, P, Q = ref.shape
    assert tuple(logits.shape) == (Bf, P, Q) and P == 60
    live = np.broadcast_to(g["query_mask"][:, None, :], ref.shape)
    scale = g["scale"][..., None]
    tol = model_tolerance(scale, ref / scale, head["logit_shift.weight"], head["logit_scale.weight"])
    lg = logits.cpu().double().numpy()
    ratio = np.where(live, np.abs(lg - ref) / tol, 0.0)
    cx, cy, w, h = (g["pred_boxes"][..., k] for k in range(4))
    corners = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    eb = float(np.abs(boxes.cpu().numpy() - corners).max())
    print(f"RECT detect vs HF at {hw}: max |d logit| {float(np.abs(lg - ref)[live].max()):.3e}, worst err / tol {ratio.max():.3f}; max |d boxes| {eb:.3e} (bar {D_BOXES})")
    assert np.array_equal(lg[~live], np.full_like(lg[~live], float(torch.finfo(torch.float32).min))) and int((~live).sum()) > 0
    assert ratio.max() <= 1.0 and eb < D_BOXES


def test_open_vocab_and_bank_steps_post_process_and_map_run_at_a_rectangle(f18):
    head = {k: f18["head/" + k] for k in weights.LOGIT_HEAD_KEYS}
    model = load_model(LABELMAP, DEV, arch="tiny", state=weights.make_weights(get_config("tiny")), image_size=(96, 160), logit_head=head)
    cfg = model.cfg
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1)
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, max_boxes=5)
    lab = [torch.from_numpy(x).to(DEV) for x in labels]; box = [torch.from_numpy(x).to(DEV) for x in boxes]
    # one forward_queries + OpenVocabLoss step
    q = torch.from_numpy(f18["query_embeds"]).to(DEV).requires_grad_(True)
    mask = torch.from_numpy(f18["query_mask"])
    p0 = model.flat_param.clone()
    opt.zero_grad()
    pb, lg = model.forward_queries(img, q, mask)
    assert tuple(pb.shape) == (B, 60, 4) and tuple(lg.shape) == (B, 60, 5)
    targets = [{"class_labels": torch.tensor([0, 2]), "boxes": torch.tensor([[0.1, 0.2, 0.5, 0.6], [0.3, 0.3, 0.9, 0.8]])} for _ in range(B)]
    out = OpenVocabLoss()(lg, pb, targets, query_mask=mask)
    (out["loss_ce"] + 5.0 * out["loss_bbox"] + 2.0 * out["loss_giou"]).backward()
    opt.step()
    model.finish()
    p1 = model.flat_param.clone()
    assert all(bool(torch.isfinite(out[k])) for k in ("loss_ce", "loss_bbox", "loss_giou")) and not torch.equal(p0, p1) and float(q.grad.abs().max()) > 0
    # one PushPullLoss step
    opt.zero_grad()
    pb, _, ps, _ = model(img)
    l = PushPullLoss(cfg.n_classes, None)(ps, lab, pb, box)
    sum(l[k] for k in LOSSES).backward()
    opt.step()
    model.finish()
    assert all(bool(torch.isfinite(l[k])) for k in LOSSES) and not torch.equal(p1, model.flat_param)
    # PostProcess and the metric take the outputs; boxes are normalised per axis, so the pixel sizes are the image's own two sides
    with torch.no_grad():
        pb, _, ps, _ = model(img)
    pp = PostProcess(0.01, 0.6)
    bx, cl, sc = pp(pb, ps, top_k=60)
    G = max(len(x) for x in labels)
    gt_boxes, gt_labels = torch.zeros(B, G, 4), torch.full((B, G), -1, dtype=torch.int64)
    for b in range(B):
        gt_boxes[b, :len(labels[b])] = torch.from_numpy(boxes[b])
        gt_labels[b, :len(labels[b])] = torch.from_numpy(np.asarray(labels[b], dtype=np.int64))
    metric = MeanAveragePrecision(iou_type="bbox", class_metrics=True, n_classes=cfg.n_classes).to(DEV)
    metric.update_batched(bx, cl, sc, pp.last_counts, gt_boxes.to(DEV), gt_labels.to(DEV), torch.tensor([len(x) for x in labels], dtype=torch.int32, device=DEV),
                          width=160.0, height=96.0)
    res = metric.compute()
    assert int(pp.last_counts.sum()) > 0 and bool(torch.isfinite(res["map"]) | (res["map"] == -1))


# ---- input stage ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(96, 160), (160, 96)], ids=["96x160", "160x96"])
def test_device_image_processor_at_a_rectangle_is_pillows_resize_plus_the_table(hw):
    H, W = hw
    rng = np.random.default_rng(18)
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((37, 53), (200, 120), (96, 160))]          # up, down and mixed; one already H x W at (96, 160)
    lut = O.normalize_lut()
    want = np.stack([np.stack([lut[c][O.pil_resize_bicubic_u8(im, H, W)[..., c]] for c in range(3)]) for im in imgs])
    for dtype in (torch.float32, torch.bfloat16):
        proc = DeviceImageProcessor(size=hw, device=DEV, dtype=dtype)
        assert proc.size == hw and proc.hw == hw
        out = proc(imgs)["pixel_values"]
        torch.cuda.synchronize()
        assert tuple(out.shape) == (3, 3, H, W) and out.dtype == dtype
        ref = torch.from_numpy(want) if dtype == torch.float32 else torch.from_numpy(want).bfloat16()
        assert np.array_equal(out.cpu().float().numpy(), ref.float().numpy())
        same = torch.from_numpy(np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)])).to(DEV)
        ns = proc.normalize_sized(same, chw=False)
        assert torch.equal(ns, proc([same[0], same[1]])["pixel_values"])


def test_a_prefetcher_fed_step_is_bitwise_the_hbm_resident_one():
    hw = (96, 160)
    Wnp = weights.make_weights(get_config("tiny"))
    cfg = _rect_cfg("tiny", hw)[1]
    u8 = torch.from_numpy(synth.make_images_u8(cfg, B, layout="hwc"))
    assert tuple(u8.shape) == (B, 96, 160, 3)
    fed = None
    for batch in DevicePrefetcher([(u8,)], DEV, size=hw, dtype=torch.bfloat16):
        assert fed is None
        fed = batch[0]
    assert tuple(fed.shape) == (B, 3, 96, 160) and fed.dtype == torch.bfloat16
    resident = DeviceImageProcessor(size=hw, device=DEV, dtype=torch.bfloat16).normalize_sized(u8.to(DEV), chw=False)
    assert torch.equal(fed, resident)
    res = []
    for img in (fed, resident):
        model = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=hw, trainable=TS.EVERYTHING)
        res.append(_step(model, img))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][3].abs().max()) > 0


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    Wnp = weights.make_weights(get_config("tiny"))
    model = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=(96, 160))
    with pytest.raises(ValueError, match=r"image must be \[B,3,96,160\]"):
        model(torch.zeros(1, 3, 160, 96, device=DEV))
    with pytest.raises(ValueError, match=r"pixel_values must be \[B, 3, 96, 160\]"):
        check_detect_args(model.cfg, torch.zeros(1, 3, 96, 96), torch.zeros(2, 64))
    with pytest.raises(ValueError, match="the width 150 is not a positive multiple of the patch size 16.*144 and 160"):
        load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=(96, 150))
    with pytest.raises(ValueError, match="8256 patches.*at most 8192"):
        load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=(16 * 129, 16 * 64))
    with pytest.raises(ValueError, match="set pos_grid"):
        OwlViT(get_config("tiny").replace(image_size=(96, 160)), Wnp, DEV)
    with pytest.raises(ValueError, match="not square"):
        model.cfg.grid
    proc = DeviceImageProcessor(size=(96, 160), device=DEV)
    img = np.zeros((50, 70, 3), np.uint8)
    with pytest.raises(ValueError, match="slices takes a square size"):
        proc.slices([img])
    with pytest.raises(ValueError, match="tiles takes a square size"):
        proc.tiles([img], [], 1)
    with pytest.raises(ValueError, match="TrainAugment takes a square size"):
        TrainAugment((96, 160))
    with pytest.raises(ValueError, match=r"DevicePrefetcher\(augment=\) takes a square size"):
        DevicePrefetcher([], DEV, size=(96, 160), augment=TrainAugment(96))
    with pytest.raises(ValueError, match="expected 96 x 160 RGB images"):
        proc.normalize_sized(torch.zeros(1, 160, 96, 3, dtype=torch.uint8, device=DEV), chw=False)
