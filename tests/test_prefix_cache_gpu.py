"""-m gpu: `model(image, image_ids=ids)` with the frozen-prefix activation cache against a twin model without one, on the same batches.

The feature claims unchanged bits, so every comparison is torch.equal: pred_boxes, pred_sims, the four losses and flat_grad, step by step.  Configs:
`tiny` (12 layers, layer 11 trains: the boundary is layer 11's first LayerNorm) and `tiny-l14` (14 layers: frozen layers 12 and 13 lie above the trainable
one and are crossed by the backward), batch 5 (two sub-batch streams, uneven split; a 3-image miss batch runs on one).  A pool of ten fixed images; an
image's id is its pool index plus an offset past 2^31."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402

DEV = "cuda"
POOL = 10
ID0 = 2 ** 31 + 5
HEADS = ("box", "post_layernorm", "class_predictor", "queries")
EVERYTHING = ("backbone", "post_post_layernorm", "class_predictor", "box_head", "queries")
LOSSES = ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")
_pool = {}

COLD, WARM, MIXED = [0, 1, 2, 3, 4], [3, 0, 4, 2, 1], [5, 1, 6, 3, 7]          # WARM: another order than when filled; MIXED: hits at 1 and 3 between three misses


def _data(cname):
    """(weights, images [POOL,3,S,S] on the device, labels, boxes): made once per config and left unchanged."""
    if cname not in _pool:
        cfg = get_config(cname)
        labels, boxes = synth.make_targets(cfg, POOL, max_boxes=5)
        _pool[cname] = (weights.make_weights(cfg), torch.from_numpy(synth.make_images(cfg, POOL)).to(DEV),
                        [torch.from_numpy(x).to(DEV) for x in labels], [torch.from_numpy(x).to(DEV) for x in boxes])
    return _pool[cname]


def _model(cname, cache=True, **kw):
    cfg = get_config(cname)
    model = OwlViT(cfg, _data(cname)[0], DEV, **kw)
    if cache is not False:
        model.enable_prefix_cache(**(cache if isinstance(cache, dict) else {}))
    return model


def _ids(idx):
    return [ID0 + i for i in idx]


def _step(model, cname, idx, ids=False, image="pool", grad=True):
    """One forward (+ loss and backward) on pool images `idx` -> (boxes, sims, losses [4], flat_grad).  ids: pass image_ids; image: "pool", "zeros" or None."""
    _, pool, labels, boxes = _data(cname)
    cfg = model.cfg
    img = pool[idx] if image == "pool" else (torch.zeros(len(idx), 3, cfg.image_size, cfg.image_size, device=DEV) if image == "zeros" else None)
    kw = dict(image_ids=_ids(idx)) if ids else {}
    if not grad:
        with torch.no_grad():
            pb, _, ps, _ = model(img, **kw)
        torch.cuda.synchronize()
        return pb.clone(), ps.clone(), None, None
    model.finish()
    model.flat_grad.zero_()
    pb, _, ps, _ = model(img, **kw)
    l = PushPullLoss(cfg.n_classes, None)(ps, [labels[i] for i in idx], pb, [boxes[i] for i in idx])
    (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
    model.finish()
    torch.cuda.synchronize()
    return pb.detach().clone(), ps.detach().clone(), torch.stack([l[k].detach() for k in LOSSES]), model.flat_grad.clone()


def _same(a, b, tag):
    for x, y, what in zip(a, b, ("pred_boxes", "pred_sims", "losses", "flat_grad")):
        assert (x is None) == (y is None), (tag, what)
        if x is not None:
            assert torch.isfinite(x).all(), (tag, what)
            assert torch.equal(x, y), (tag, what, float((x - y).abs().max()))


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_every_step_is_bitwise_the_uncached_step(cname):
    model, twin = _model(cname), _model(cname, cache=False)
    assert model._chain_low == 11
    for tag, idx in (("cold", COLD), ("warm", WARM), ("mixed", MIXED), ("an id three times, one twice", [8, 8, 2, 9, 8])):
        _same(_step(model, cname, idx, ids=True), _step(twin, cname, idx), f"{cname} {tag}")
    s = model.prefix_cache.stats
    # cold 5 misses; warm 5 hits; mixed 2 hits + 3 misses; last: id 2 hit, ids 8 and 9 computed once each, 8's two later positions copied
    assert (s["hits"], s["misses"], s["admitted"], s["refused"], s["duplicates"], s["slots"]) == (8, 10, 10, 0, 2, 10)
    pc, E = model.prefix_cache, model.cfg.tokens_padded * model.cfg.hidden
    # slots live in slabs allocated whole: ten tiny images sit in the first one
    assert s["bytes"] == pc.nbytes == min(pc.capacity, pc.slab_slots) * 4 * E and 10 * 4 * E <= pc.nbytes <= pc.max_bytes
    assert model.prefix_cache.contains(_ids(range(POOL))) == [True] * POOL


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_a_budget_of_three_slots(cname):
    cfg = get_config(cname)
    E = cfg.tokens_padded * cfg.hidden
    model, twin = _model(cname, cache=dict(max_bytes=3 * 4 * E + 100)), _model(cname, cache=False)
    _same(_step(model, cname, COLD, ids=True), _step(twin, cname, COLD), "cold: three admitted, two refused")
    assert model.prefix_cache.contains(_ids(COLD)) == [True, True, True, False, False]
    _same(_step(model, cname, WARM, ids=True), _step(twin, cname, WARM), "three hits, the refused two computed again")
    _same(_step(model, cname, WARM, ids=True, grad=False), _step(twin, cname, WARM, grad=False), "the same, no-grad")
    s = model.prefix_cache.stats
    assert (s["hits"], s["misses"], s["admitted"], s["refused"], s["slots"]) == (6, 9, 3, 6, 3)
    assert s["bytes"] == 3 * 4 * E <= model.prefix_cache.max_bytes
    model2 = _model(cname, cache=dict(max_images=3))
    _step(model2, cname, COLD, ids=True, grad=False)
    assert model2.prefix_cache.stats["slots"] == 3 and model2.prefix_cache.stats["refused"] == 2


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_consecutive_optimizer_steps(cname, overlap):
    """The trainable layer moves, the prefix does not: states kept at step 1 serve steps 2 and 3, in line and with the backward / AdamW deferred under the
    next forward (whose kept-state hand-over then has to wait for that tail before it writes what the backward reads)."""
    model, twin = _model(cname), _model(cname, cache=False)
    _, pool, labels, boxes = _data(cname)
    opts = [FusedAdamW(m, lr=1e-3, weight_decay=0.1, overlap=overlap) for m in (model, twin)]
    crit = PushPullLoss(model.cfg.n_classes, None)
    for tag, idx in (("cold", COLD), ("mixed", MIXED), ("warm", [7, 4, 6, 0, 5])):
        outs = []
        for m, opt in zip((model, twin), opts):
            opt.zero_grad()
            pb, _, ps, _ = m(pool[idx], image_ids=_ids(idx)) if m is model else m(pool[idx])
            l = crit(ps, [labels[i] for i in idx], pb, [boxes[i] for i in idx])
            (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
            m.finish()
            grad = m.flat_grad.clone()
            opt.step()
            outs.append((pb.detach().clone(), ps.detach().clone(), torch.stack([l[k].detach() for k in LOSSES]), grad))
        torch.cuda.synchronize()
        _same(outs[0], outs[1], f"{cname} overlap={overlap} {tag}")
    model.finish(); twin.finish()
    torch.cuda.synchronize()
    assert torch.equal(model.flat_param, twin.flat_param)
    assert model.prefix_cache.stats["hits"] == 2 + 5


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_the_prefix_really_is_skipped(cname):
    model = _model(cname)
    ref = _step(model, cname, COLD, ids=True)
    ref_eval = _step(model, cname, COLD, ids=True, grad=False)
    # other pixels under the same ids: the outputs are those of the original images, so nothing below the boundary read the tensor
    _same(_step(model, cname, COLD, ids=True, image="zeros"), ref, "zeros image, training step")
    _same(_step(model, cname, COLD, ids=True, image="zeros", grad=False), ref_eval, "zeros image, no-grad")
    zeros_uncached = _step(model, cname, COLD, image="zeros", grad=False)
    assert not torch.equal(zeros_uncached[0], ref_eval[0])          # (the zeros image does give other outputs where it is read)
    # no image at all
    _same(_step(model, cname, WARM, ids=True, image=None), _step(model, cname, WARM, ids=True), "image=None, training step")
    _same(_step(model, cname, WARM, ids=True, image=None, grad=False), _step(model, cname, WARM, ids=True, grad=False), "image=None, no-grad")
    before = dict(model.prefix_cache.stats)
    with pytest.raises(ValueError, match=str(ID0 + 6)) as e:
        model(None, image_ids=_ids(MIXED))
    assert str(ID0 + 5) in str(e.value) and str(ID0 + 7) in str(e.value) and str(ID0 + 1) not in str(e.value)
    with pytest.raises(ValueError):
        model(None)
    assert model.prefix_cache.stats == before          # a refused call counts nothing and keeps nothing
    assert (before["hits"], before["misses"], before["slots"]) == (7 * 5, 5, 5)
    # ids are host integers: a device tensor would have to be read back
    with pytest.raises(TypeError, match="device tensor"):
        model(None, image_ids=torch.tensor(_ids(COLD), device=DEV))
    with pytest.raises(ValueError, match="entries"):
        model(_data(cname)[1][COLD], image_ids=_ids(COLD)[:4])


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_eval_and_train_share_the_slots(cname):
    twin = _model(cname, cache=False)
    model = _model(cname)
    _same(_step(model, cname, COLD, ids=True, grad=False), _step(twin, cname, COLD, grad=False), "filled under no_grad")
    _same(_step(model, cname, WARM, ids=True), _step(twin, cname, WARM), "... hit by a training step")
    assert model.prefix_cache.stats["misses"] == 5 and model.prefix_cache.stats["hits"] == 5
    model = _model(cname)
    _same(_step(model, cname, MIXED, ids=True), _step(twin, cname, MIXED), "filled by a training step")
    _same(_step(model, cname, [7, 5, 9, 6, 3], ids=True, grad=False), _step(twin, cname, [7, 5, 9, 6, 3], grad=False), "... hit under no_grad, one miss between")
    assert model.prefix_cache.stats["misses"] == 6 and model.prefix_cache.stats["hits"] == 4


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_a_heads_only_set_keeps_the_state_behind_the_encoder(cname):
    model, twin = _model(cname, trainable=HEADS), _model(cname, cache=False, trainable=HEADS)
    assert model._chain_low is None
    for tag, idx in (("cold", COLD), ("warm", WARM), ("mixed", MIXED)):
        _same(_step(model, cname, idx, ids=True), _step(twin, cname, idx), f"heads only, {tag}")
        _same(_step(model, cname, idx, ids=True, grad=False), _step(twin, cname, idx, grad=False), f"heads only, {tag}, no-grad")
    _same(_step(model, cname, WARM, ids=True, image="zeros"), _step(twin, cname, WARM), "heads only: no encoder layer reads the image")
    assert model.prefix_cache.stats["misses"] == 8


@pytest.mark.parametrize("keep", [EVERYTHING, ("backbone.embeddings",), ("pre_layernorm", "layers.11."), ("layers.0.", "queries")])
def test_a_set_without_a_frozen_prefix_is_refused(keep):
    model = _model("tiny", cache=False, trainable=keep)
    with pytest.raises(ValueError, match="no frozen prefix") as e:
        model.enable_prefix_cache()
    assert keep[0] in str(e.value)          # the message names the trainable set
    assert model.prefix_cache is None


def test_whatever_may_change_a_frozen_tensor_empties_the_cache():
    """load_state_dict with other frozen weights: the next outputs are a fresh model's.  The frozen tensors changed here are the ones a forward reads where
    they lie (LayerNorm affines and biases of the prefix); the bf16 copies of frozen GEMM weights are made at construction and load_state_dict does not
    re-make them, with or without this cache."""
    cname = "tiny"
    model = _model(cname)
    ref = _step(model, cname, COLD, ids=True, grad=False)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    changed = ["backbone.pre_layernorm.weight", "backbone.pre_layernorm.bias", "backbone.encoder.layers.0.layer_norm1.weight", "backbone.encoder.layers.3.mlp.fc2.bias",
               "backbone.encoder.layers.10.self_attn.out_proj.bias", "backbone.encoder.layers.10.layer_norm2.bias"]
    for n in changed:
        sd[n] = sd[n] + 0.05 * torch.randn(sd[n].shape, generator=g).to(DEV)
    model.load_state_dict(sd)
    assert len(model.prefix_cache) == 0 and model.prefix_cache.nbytes == 0 and model.prefix_cache.contains(_ids(COLD)) == [False] * 5
    fresh = OwlViT(model.cfg, {k: v.cpu().numpy() for k, v in sd.items()}, DEV)
    want = _step(fresh, cname, COLD, grad=False)
    got = _step(model, cname, COLD, ids=True, grad=False)
    _same(got, want, "after load_state_dict")
    assert not torch.equal(got[0], ref[0])
    _same(_step(model, cname, WARM, ids=True), _step(fresh, cname, WARM), "and the refilled slots serve the new weights")
    # the other doors
    assert len(model.prefix_cache) == 5
    model.refresh_compute_weights(force=True)
    assert len(model.prefix_cache) == 0
    _step(model, cname, COLD, ids=True, grad=False)
    model.to(DEV)
    assert len(model.prefix_cache) == 0
    _step(model, cname, COLD, ids=True, grad=False)
    model.prefix_cache.clear()
    assert len(model.prefix_cache) == 0 and model.prefix_cache.stats["misses"] == 20
    # another input size is another model: its cache is its own, keyed to its config
    assert model.prefix_cache.key == model.cfg and model.prefix_cache.block_elems == model.cfg.tokens_padded * model.cfg.hidden


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14"])
def test_off_means_off(cname):
    twin = _model(cname, cache=False)
    want, want_eval = _step(twin, cname, COLD), _step(twin, cname, COLD, grad=False)
    model = _model(cname)
    _same(_step(model, cname, COLD), want, "cache enabled, image_ids=None")
    _same(_step(model, cname, COLD, grad=False), want_eval, "cache enabled, image_ids=None, no-grad")
    assert model.prefix_cache.stats["misses"] == 0 and model.prefix_cache.nbytes == 0
    _step(model, cname, COLD, ids=True)
    _same(_step(model, cname, COLD), want, "between cached steps")
    model.disable_prefix_cache()
    assert model.prefix_cache is None
    _same(_step(model, cname, COLD), want, "cache disabled")
    with pytest.raises(RuntimeError, match="enable_prefix_cache"):
        model(_data(cname)[1][COLD], image_ids=_ids(COLD))
