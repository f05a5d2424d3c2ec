"""-m gpu: a model built at another input size than its position table's -- `load_model(..., image_size=)` / `OwlViT(cfg)` with `cfg.pos_grid` set.

`tiny` (native 96, a 6 x 6 table) runs at 128 (T = 65: T - 1 = 64 is the first size at which the class-token-peeled attention variant is eligible on this
config), 160 (T = 101 in Tp = 104: the plain variant with a ragged tail) and 64 (T = 17: a shrink); `tiny-p14` of tests/test_trainable_sets_gpu.py (84,
14-pixel patches) runs at 112.  The oracle is called UNCHANGED with `cfg.replace(image_size=S)` and a state whose position table is the float64
tap-matrix reference's table (tests/pos_resample_reference.py) cast to f32; the expected gradient of the native table is that reference's adjoint applied
to the oracle's gradient of the table it was handed.  Bounds: the ones tests/test_model_gpu.py asserts for these configs at the native size (outputs) and
the project's gradient band (rel-L2 < 2e-2, cosine > 0.9995)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import owl_oracle as O  # noqa: E402  (checker only)
from owl_vit_object_detection_amd import synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT, load_model  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from tests import pos_resample_reference as R  # noqa: E402
from tests import test_trainable_sets_gpu as TS  # noqa: E402  (its gradient measure, band and the tiny-p14 config)
from tests.test_model_gpu import TOL_BOXES, TOL_SIMS_SMALLCFG  # noqa: E402

DEV = "cuda"
POS = "backbone.embeddings.position_embedding.weight"
LABELMAP = {i: f"c{i}" for i in range(4)}
CASES = [("tiny", 128), ("tiny", 160), ("tiny", 64), ("tiny-p14", 112)]
B = 2
_ref_cache = {}


def _native(cname):
    return TS._cfg(cname)


def _build(cname, S, state, **kw):
    """`tiny` through load_model(image_size=) -- the native grid read off the state's table --, `tiny-p14` (no named architecture) through OwlViT(cfg)."""
    cfg0 = _native(cname)
    if cname == "tiny":
        return load_model(LABELMAP, DEV, arch="tiny", state=state, image_size=S, **kw)
    return OwlViT(cfg0.replace(image_size=S, pos_grid=cfg0.grid), state, DEV, **kw)


def _reference(cname, S):
    """Once per (config, size): native weights, images at S, a fixed upstream, the oracle's outputs and gradients at S on the float64-resampled table."""
    if (cname, S) in _ref_cache:
        return _ref_cache[(cname, S)]
    cfg0 = _native(cname)
    cfg = cfg0.replace(image_size=S)                      # what the oracle sees: a model whose table was drawn at S
    g0, g = cfg0.grid, cfg.grid
    Wnp = weights.make_weights(cfg0)
    img = synth.make_images(cfg, B)
    w = {k: torch.from_numpy(v) for k, v in Wnp.items()}
    w[POS] = R.forward64(w[POS], g0, g).float()
    gen = torch.Generator().manual_seed(5)
    d_boxes = torch.randn(B, cfg.patches, 4, generator=gen) * 0.1
    d_sims = torch.randn(B, cfg.patches, cfg.n_classes, generator=gen) * 0.1
    ww = {n: t.clone().requires_grad_(True) for n, t in w.items()}
    taps = {}
    rb, rs = O.model_forward(cfg, ww, torch.from_numpy(img), taps)
    with torch.no_grad():          # near-tie prompt routes get no upstream (the recipe of tests/test_trainable_sets_gpu.py::_reference)
        e = torch.nn.functional.linear(taps["feats"], w["class_predictor.dense0.weight"], w["class_predictor.dense0.bias"])
        e = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
        q = w["queries"] / torch.linalg.norm(w["queries"], dim=-1, keepdim=True) + 1e-6
        top2 = (e @ q.transpose(1, 2)).view(B, cfg.patches, cfg.n_classes, 3).topk(2, dim=-1).values
        d_sims = d_sims * ((top2[..., 0] - top2[..., 1]) > 0.02).float()
    torch.autograd.backward([rb, rs], [d_boxes, d_sims])
    gref = {n: ww[n].grad.detach() for n in ww}
    gref[POS] = R.adjoint64(gref[POS], g0, g).float()     # K^T in float64 on the oracle's gradient of the table it was handed
    out = dict(Wnp=Wnp, img=img, d_boxes=d_boxes, d_sims=d_sims, rb=rb.detach(), rs=rs.detach(), gref=gref, cfg=cfg, g0=g0, g=g)
    _ref_cache[(cname, S)] = out
    return out


@pytest.mark.parametrize("cname,S", CASES)
def test_forward_with_frozen_embeddings_matches_the_oracle(cname, S):
    r = _reference(cname, S)
    model = _build(cname, S, r["Wnp"])
    cfg = model.cfg
    assert cfg.image_size == S and cfg.grid == r["g"] and cfg.native_grid == r["g0"] and not model._train_emb
    assert tuple(model.p(POS).shape) == (r["g0"] ** 2 + 1, cfg.hidden) and tuple(model._pos_used.shape) == (cfg.tokens, cfg.hidden)
    with torch.no_grad():
        pb, _, ps, _ = model(torch.from_numpy(r["img"]).to(DEV))
    assert pb.shape == (B, cfg.patches, 4) and ps.shape == (B, cfg.patches, cfg.n_classes)
    eb, es = float((pb.cpu() - r["rb"]).abs().max()), float((ps.cpu() - r["rs"]).abs().max())
    print(f"{cname} at {S} (T = {cfg.tokens}): max|d boxes|={eb:.3e} max|d sims|={es:.3e}")
    assert eb < TOL_BOXES and es < TOL_SIMS_SMALLCFG, (eb, es)


@pytest.mark.parametrize("cname,S", CASES)
def test_gradients_of_a_full_fine_tune_match_the_oracle(cname, S):
    r = _reference(cname, S)
    model = _build(cname, S, r["Wnp"], trainable=TS.EVERYTHING)
    pb, _, ps, _ = model(torch.from_numpy(r["img"]).to(DEV))
    torch.autograd.backward([pb, ps], [r["d_boxes"].to(DEV), r["d_sims"].to(DEV)])
    torch.cuda.synchronize()
    names = list(weights.param_shapes(model.cfg))
    assert set(names) == set(model.flat_offsets)
    grads = {n: model.p(n).grad.detach().float().cpu() for n in names}
    assert tuple(grads[POS].shape) == (r["g0"] ** 2 + 1, model.cfg.hidden)          # the native shape
    worst, worst_cos = TS._grad_report(grads, {n: r["gref"][n] for n in names}, f"everything {cname} at {S}")
    assert worst < TS.REL_L2 and worst_cos > TS.COS, (worst, worst_cos)
    w, c = TS._grad_report({POS: grads[POS]}, {POS: r["gref"][POS]}, f"everything {cname} at {S}: {POS}")
    assert w < TS.REL_L2 and c > TS.COS, (w, c)


def test_native_size_through_the_keyword_is_bitwise_the_model_without_it():
    cfg = get_config("tiny")
    Wnp = weights.make_weights(cfg)
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    gen = torch.Generator().manual_seed(5)
    d_boxes = (torch.randn(B, cfg.patches, 4, generator=gen) * 0.1).to(DEV)
    d_sims = (torch.randn(B, cfg.patches, cfg.n_classes, generator=gen) * 0.1).to(DEV)
    res = []
    for kw in ({}, {"image_size": 96}):
        model = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, trainable=TS.EVERYTHING, **kw)
        assert model._pos_used is None and model.cfg == cfg.replace(n_classes=4)          # nothing of the resampler exists
        pb, _, ps, _ = model(img)
        torch.autograd.backward([pb, ps], [d_boxes, d_sims])
        torch.cuda.synchronize()
        res.append((pb.detach().clone(), ps.detach().clone(), model.flat_grad.clone(), list(model.flat_offsets.items())))
    assert res[0][3] == res[1][3]
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert float(res[0][2].abs().max()) > 0


def _train(model, steps, overlap, lr=1e-3):
    cfg = model.cfg
    labels, boxes = synth.make_targets(cfg, 4, max_boxes=5)
    lab = [torch.from_numpy(x).to(DEV) for x in labels]; box = [torch.from_numpy(x).to(DEV) for x in boxes]
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=lr, weight_decay=0.1, overlap=overlap)
    gen = torch.Generator(device="cpu").manual_seed(7)
    imgs = [torch.randn(4, 3, cfg.image_size, cfg.image_size, generator=gen).to(DEV) for _ in range(steps)]
    hist = []
    for s in range(steps):
        opt.zero_grad()
        pb, _, ps, _ = model(imgs[s])
        l = crit(ps, lab, pb, box)
        loss = l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]
        loss.backward()
        hist.append(loss.detach())
        opt.step()
    model.finish()
    torch.cuda.synchronize()
    return opt, torch.stack(hist).cpu(), imgs


def test_the_used_table_follows_the_parameter_through_optimizer_steps():
    """Three FusedAdamW steps at 128 with trainable embeddings: the next no-grad forward must be the forward of a FRESH model built from the stepped
    state_dict() -- a table resampled before the steps (stale) would not be."""
    Wnp = weights.make_weights(get_config("tiny"))
    model = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=128, trainable=TS.EVERYTHING)
    before = model.p(POS).detach().clone()
    _, hist, imgs = _train(model, 3, overlap=False, lr=1e-2)
    assert bool(torch.isfinite(hist).all())
    assert not torch.equal(before, model.p(POS).detach()), "the steps did not move the position table: the check below would be vacuous"
    with torch.no_grad():
        pb, _, ps, _ = model(imgs[0])
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    assert tuple(sd[POS].shape) == (37, 128)
    fresh = load_model(LABELMAP, DEV, arch="tiny", state=sd, image_size=128, trainable=TS.EVERYTHING)
    with torch.no_grad():
        fb, _, fs, _ = fresh(imgs[0])
    torch.cuda.synchronize()
    assert torch.equal(pb, fb) and torch.equal(ps, fs)
    # frozen embeddings: load_state_dict rebuilds the used table
    frozen = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=128)
    stale = frozen._pos_used.clone()
    frozen.load_state_dict(model.state_dict())
    torch.cuda.synchronize()
    assert not torch.equal(stale, frozen._pos_used) and torch.equal(frozen._pos_used, fresh._pos_used)


def test_deferred_tail_at_another_size_is_bitwise_the_inline_schedule():
    out = []
    for overlap in (False, True):
        model = load_model(LABELMAP, DEV, arch="tiny", state=weights.make_weights(get_config("tiny")), image_size=128, trainable=TS.EVERYTHING)
        _, hist, _ = _train(model, 3, overlap=overlap)
        assert model.overlap_tail == overlap
        out.append((hist, model.flat_param.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][0]).all())


def test_optimizer_state_written_at_one_size_loads_at_another():
    Wnp = weights.make_weights(get_config("tiny"))
    m96 = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, trainable=TS.EVERYTHING)
    opt96, _, _ = _train(m96, 1, overlap=False)
    m128 = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=128, trainable=TS.EVERYTHING)
    assert list(m96.flat_offsets.items()) == list(m128.flat_offsets.items()) and m96.flat_numel == m128.flat_numel
    opt = FusedAdamW(m128, lr=1e-3, weight_decay=0.1)
    opt.load_state_dict(opt96.state_dict())
    assert opt.step_count == 1 and torch.equal(opt.exp_avg, opt96.exp_avg)
    m128.load_state_dict(m96.state_dict())          # ... and so does the model's own state dict
    assert torch.equal(m128.flat_param, m96.flat_param)


def test_errors():
    Wnp = weights.make_weights(get_config("tiny"))
    model = load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=128)
    with pytest.raises(ValueError, match=r"image must be \[B,3,128,128\]"):
        model(torch.zeros(1, 3, 96, 96, device=DEV))
    with pytest.raises(ValueError, match="96 and 112"):
        load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=100)
    with pytest.raises(ValueError, match="at most 8192"):
        load_model(LABELMAP, DEV, arch="tiny", state=Wnp, image_size=16 * 91)
    bad = dict(Wnp)
    bad[POS] = Wnp[POS][:36]
    with pytest.raises(ValueError, match="36 rows"):
        load_model(LABELMAP, DEV, arch="tiny", state=bad, image_size=128)
    with pytest.raises(ValueError, match="position table in `state` has 37 rows"):
        OwlViT(get_config("tiny").replace(image_size=128), Wnp, DEV)          # a config that expects a table drawn at 128
