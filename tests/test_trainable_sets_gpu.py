"""-m gpu: `OwlViT(..., trainable=[...])` -- the backward laid out for another trainable set than the reference's freeze rule.

Yardstick for gradients: the recipe of tests/test_model_gpu.py::test_backward_chain_matches_oracle_given_same_upstream -- the same random upstream
(d_boxes, d_sims) into the HIP backward and into the oracle under torch autograd, near-tie prompt routes masked, every trainable tensor compared with
that file's rel-L2 / cosine measure (restated below), bound worst rel-L2 < 2e-2 and worst cosine > 0.9995.  The oracle's gradient of a tensor does not
depend on which other tensors require one, so one oracle backward per (config, batch) with EVERY parameter recording serves all cases of that shape.
Every case prints its worst figures; profiles/trainable_sets.md records them.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import owl_oracle as O  # noqa: E402  (checker only)
from owl_vit_object_detection_amd import autograd, ops, synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402

DEV = "cuda"
HEADS = ("box", "post_layernorm", "class_predictor", "queries")
EVERYTHING = ("backbone", "post_post_layernorm", "class_predictor", "box_head", "queries")
REL_L2, COS = 2e-2, 0.9995          # the project's own band (tests/test_model_gpu.py:216)
_ref_cache = {}
# a patch size that is not 2^n at test size: 84 x 84 pixels in 14-pixel patches (patch_k = 588; the forward's patch embedding at this shape is a case of
# tests/test_kernels_gpu.py), two encoder layers
_CFGS = {"tiny-p14": get_config("tiny").replace(name="tiny-p14", image_size=84, patch_size=14, layers=2)}


def _cfg(cname):
    return _CFGS.get(cname) or get_config(cname)


def _grad_report(grads, ref, tag):
    """rel-L2 per tensor, measured against max(|ref|, 1e-3 * largest |ref|): tensors whose true gradient
    is ~0 (k_proj.bias: softmax is invariant to a key bias) are judged on an absolute scale."""
    floor = 1e-3 * max(float(r.float().norm()) for r in ref.values())
    worst, worst_cos = 0.0, 1.0
    lines = []
    for n, r in ref.items():
        g = grads[n]
        r = r.float()
        rel = float((g - r).norm() / max(float(r.norm()), floor))
        cos = float((g * r).sum() / (g.norm() * r.norm() + 1e-20)) if float(r.norm()) > floor else 1.0
        lines.append(f"  {n:58s} rel_l2={rel:.3e} cos={cos:.5f} |ref|={float(r.norm()):.3e}")
        worst = max(worst, rel)
        worst_cos = min(worst_cos, cos)
    print(f"[{tag}] worst rel-L2 grad error {worst:.3e}, worst cos {worst_cos:.5f}\n" + "\n".join(lines))
    return worst, worst_cos


def _reference(cname, B):
    """(Wnp, img, d_boxes, d_sims, {name: oracle gradient}) for every parameter, computed once per shape and left unchanged."""
    if (cname, B) in _ref_cache:
        return _ref_cache[(cname, B)]
    cfg = _cfg(cname)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    Wnp = weights.make_weights(cfg)
    img = synth.make_images(cfg, B)
    g = torch.Generator().manual_seed(5)
    d_boxes = torch.randn(B, cfg.patches, 4, generator=g) * 0.1
    d_sims = torch.randn(B, cfg.patches, cfg.n_classes, generator=g) * 0.1
    w = {k: torch.from_numpy(v) for k, v in Wnp.items()}
    ww = {n: t.clone().requires_grad_(True) for n, t in w.items()}
    taps = {}
    rb, rs = O.model_forward(cfg, ww, torch.from_numpy(img), taps)
    # MaxPool1d(3) routes each class gradient to ONE of three prompts; where the top two prompts are within
    # bf16 forward noise of each other the routing is a coin flip, so those (row, class) pairs get no upstream
    with torch.no_grad():
        e = torch.nn.functional.linear(taps["feats"], w["class_predictor.dense0.weight"], w["class_predictor.dense0.bias"])
        e = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
        q = w["queries"] / torch.linalg.norm(w["queries"], dim=-1, keepdim=True) + 1e-6
        top2 = (e @ q.transpose(1, 2)).view(B, cfg.patches, cfg.n_classes, 3).topk(2, dim=-1).values
        d_sims = d_sims * ((top2[..., 0] - top2[..., 1]) > 0.02).float()
    torch.autograd.backward([rb, rs], [d_boxes, d_sims])
    out = (Wnp, img, d_boxes, d_sims, {n: ww[n].grad.detach() for n in ww})
    _ref_cache[(cname, B)] = out
    return out


def _backward_case(cname, B, keep, tag):
    """HIP backward under `trainable=keep` against the shared oracle gradients; asserts the band and that frozen tensors got no gradient."""
    cfg = _cfg(cname)
    Wnp, img, d_boxes, d_sims, gref = _reference(cname, B)
    model = OwlViT(cfg, Wnp, DEV, trainable=keep)
    pb, _, ps, _ = model(torch.from_numpy(img).to(DEV))
    torch.autograd.backward([pb, ps], [d_boxes.to(DEV), d_sims.to(DEV)])
    torch.cuda.synchronize()
    names = [n for n in weights.param_shapes(cfg) if weights.is_trainable(n, keep)]
    assert {n for n, p in model.named_parameters() if p.requires_grad} == set(names) == set(model.flat_offsets)
    for n, p in model.named_parameters():
        assert (p.grad is not None) == (n in names), n
    grads = {n: model.p(n).grad.detach().float().cpu() for n in names}
    worst, worst_cos = _grad_report(grads, {n: gref[n] for n in names}, f"{tag} {cname} B={B}")
    assert worst < REL_L2 and worst_cos > COS, (worst, worst_cos)
    return model, grads


def _layers(*idx):
    return tuple(f"layers.{i}." for i in idx)


# ---- 1. the reference set spelled out ---------------------------------------------------------------------------------------------------
def _full_step(cname, B, **kw):
    cfg = get_config(cname)
    model = OwlViT(cfg, weights.make_weights(cfg), DEV, **kw)
    img = torch.from_numpy(synth.make_images(cfg, B)).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, max_boxes=5)
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1)
    opt.zero_grad()
    pb, _, ps, _ = model(img)
    l = crit(ps, [torch.from_numpy(x).to(DEV) for x in labels], pb, [torch.from_numpy(x).to(DEV) for x in boxes])
    (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
    grad = model.flat_grad.clone()
    opt.step()
    torch.cuda.synchronize()
    return model, pb.detach().clone(), ps.detach().clone(), grad, model.flat_param.clone()


@pytest.mark.parametrize("cname,B", [("tiny", 3), ("tiny-l14", 5)])       # B = 5: two sub-batch streams, uneven split
def test_reference_set_spelled_out_is_bitwise_the_default(cname, B):
    m0, pb0, ps0, g0, p0 = _full_step(cname, B)
    m1, pb1, ps1, g1, p1 = _full_step(cname, B, trainable=weights.FREEZE_KEEP)
    assert list(m0.flat_offsets.items()) == list(m1.flat_offsets.items()) and m0.flat_numel == m1.flat_numel
    assert m1.trainable_layers == (11,) and m1.backward_floor == 11 and m0.backward_floor == 11
    assert torch.equal(pb0, pb1) and torch.equal(ps0, ps1) and torch.equal(g0, g1) and torch.equal(p0, p1)
    assert float(g0.abs().max()) > 0


# ---- 2. - 4. encoder layers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
def test_two_adjacent_trainable_layers(B):
    model, _ = _backward_case("tiny", B, _layers(10, 11) + HEADS, "layers 10 + 11")
    assert model.trainable_layers == (10, 11) and model.backward_floor == 10


def test_last_layer_only_on_the_deeper_model():
    model, _ = _backward_case("tiny-l14", 2, _layers(13) + HEADS, "layer 13 only")
    assert model.trainable_layers == (13,) and model.backward_floor == 13
    assert [k for k in model._ws if isinstance(k, tuple) and k[0] == "layer"] == [("layer", 2, 13)]          # no dX-only layer ran or was kept
    assert not any(k.endswith("T") for k in model._fz if k[0].isdigit())


def test_trainable_frozen_trainable():
    model, _ = _backward_case("tiny-l14", 2, _layers(11, 13) + HEADS, "layers 11 + 13, 12 crossed")
    assert model.trainable_layers == (11, 13) and model.backward_floor == 11
    assert sorted(k[2] for k in model._ws if isinstance(k, tuple) and k[0] == "layer") == [11, 12, 13]
    assert "12.w2T" in model._fz and "h1" not in model._ws[("layer", 2, 12)] and "h1" in model._ws[("layer", 2, 11)]


# ---- 5. queries only, heads only ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep,floor", [(("queries",), "heads"), (("queries", "class_predictor", "box"), "heads")])
def test_sets_that_stop_at_the_heads(keep, floor):
    cfg = get_config("tiny")
    model, _ = _backward_case("tiny", 3, keep, "+".join(keep))
    assert model.backward_floor == floor and model.trainable_layers == ()
    assert not any(isinstance(k, tuple) and k[0] == "layer" for k in model._ws)
    frozen = {n: p.detach().clone() for n, p in model.named_parameters() if not p.requires_grad}
    assert len(frozen) == len(weights.param_shapes(cfg)) - len(model.flat_offsets) > 0
    before = model.flat_param.clone()
    FusedAdamW(model, lr=1e-2, weight_decay=0.1).step()
    torch.cuda.synchronize()
    assert not torch.equal(before, model.flat_param)
    for n, t in frozen.items():
        assert torch.equal(model.p(n).detach(), t), n


# ---- 6. full fine-tune --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname,B", [("tiny", 1), ("tiny", 3), ("small", 2), ("owlvit-base-patch32", 1)])     # B/32: D = 768, patch_k = 3072 -> the TN route
def test_full_fine_tune(cname, B):
    cfg = get_config(cname)
    model, grads = _backward_case(cname, B, EVERYTHING, "everything")
    assert model.backward_floor == "embeddings" and model.trainable_layers == tuple(range(cfg.layers))
    assert set(grads) == set(weights.param_shapes(cfg))
    gref = _reference(cname, B)[4]
    for n in ("backbone.embeddings.position_embedding.weight", "backbone.embeddings.patch_embedding.weight", "backbone.embeddings.class_embedding",
              "backbone.pre_layernorm.weight"):
        w, c = _grad_report({n: grads[n]}, {n: gref[n]}, f"everything {cname} B={B}: {n}")
        assert w < REL_L2 and c > COS, (n, w, c)


@pytest.mark.parametrize("keep,layers,floor", [(("layers.11.", "queries"), (11,), 11), (("pre_layernorm", "layers.0."), (0,), "pre_layernorm")])
def test_chain_crosses_frozen_head_units(keep, layers, floor):
    """The dX chain runs through head units that do not train: the box head and class_predictor as dX only on their static transposed copies, the two final
    LayerNorms with their affine gradients going to the sink, box_final_bwd without dense1's bias gradient."""
    model, _ = _backward_case("tiny", 3, keep, "frozen heads crossed: " + "+".join(keep))
    assert model.trainable_layers == layers and model.backward_floor == floor
    assert "box_head.dense1.weight.T" in model._fz and "class_predictor.dense0.weight.T" in model._fz and "box_head.dense0.weight" not in model.flat_offsets


def test_full_fine_tune_with_a_patch_size_that_is_not_a_power_of_two():
    """p = 14, patch_k = 588: the patch-embedding weight gradient on the NT split-K route through the backward's shared scratch, against the oracle; then
    two optimizer steps -- the forward's gather-layout weight must follow the bucket after each (and after refresh_compute_weights)."""
    cname, B = "tiny-p14", 3
    cfg = _cfg(cname)
    model, grads = _backward_case(cname, B, EVERYTHING, "everything")
    assert model._pe_gather is not None and model.backward_floor == "embeddings"
    gref = _reference(cname, B)[4]
    for n in ("backbone.embeddings.position_embedding.weight", "backbone.embeddings.patch_embedding.weight", "backbone.embeddings.class_embedding"):
        w, c = _grad_report({n: grads[n]}, {n: gref[n]}, f"everything {cname} B={B}: {n}")
        assert w < REL_L2 and c > COS, (n, w, c)
    pe = "backbone.embeddings.patch_embedding.weight"

    def laid_out():          # what the forward's weight has to be: the bucket's bf16 copy in the gather loader's K order
        return weights.patch_weight_gather_layout(model._tview(pe).float(), cfg.patch_size).to(torch.bfloat16)

    img = torch.from_numpy(_reference(cname, B)[1]).to(DEV)
    labels, boxes = synth.make_targets(cfg, B, max_boxes=5)
    lab = [torch.from_numpy(x).to(DEV) for x in labels]; box = [torch.from_numpy(x).to(DEV) for x in boxes]
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=1e-2, weight_decay=0.1)
    for step in range(2):
        before = model._tview(pe).clone()
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        assert torch.equal(model._fz["w_pe"], laid_out()), f"step {step}: the forward ran on a stale patch-embedding weight"
        l = crit(ps, lab, pb, box)
        (l["loss_ce"] + l["loss_bg"] + l["loss_bbox"] + l["loss_giou"]).backward()
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(before, model._tview(pe)), "the step did not move the patch-embedding weight: the check above would be vacuous"
    with torch.no_grad():
        model.p(pe).data.mul_(1.5)
    model.refresh_compute_weights()
    torch.cuda.synchronize()
    assert torch.equal(model._fz["w_pe"], laid_out()) and bool(model._fz["w_pe"].any())


# ---- 7. the kernels below layer 0 alone, against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,grid,p,D", [(1, 6, 16, 128), (3, 6, 16, 128), (2, 5, 14, 128)])      # the last: K = 588, T = 26 in Tp = 32 (pad rows), patch size not 2^n
def test_embed_bwd_and_patch_weight_gradient_alone(B, grid, p, D):
    P, S, K = grid * grid, grid * p, 3 * p * p
    T = P + 1
    Tp = (T + 7) // 8 * 8
    g = torch.Generator().manual_seed(11)
    dx = torch.randn(B, Tp, D, generator=g)
    dx[:, T:] = float("nan")                                             # pad rows hold NaN: they must not leak into any sum or row
    img = torch.randn(B, 3, S, S, generator=g).to(torch.bfloat16)
    dE_all = torch.full((ops.pad_rows(B * P) + 8, D), 0x4B5A, dtype=torch.int16, device=DEV).view(torch.bfloat16)      # 8 sentinel rows behind the buffer
    dE = dE_all[:ops.pad_rows(B * P)]
    patches = torch.zeros(ops.pad_rows(B * P), (K + 7) // 8 * 8, dtype=torch.bfloat16, device=DEV)
    ops.im2row_bf16(img.to(DEV), patches, B, S, p)
    x64 = dx.double()
    ref_pos = x64[:, :T].sum(0)
    ref_dE = dx[:, 1:T].reshape(B * P, D).to(torch.bfloat16)
    ref_patches = img.view(B, 3, grid, p, grid, p).permute(0, 2, 4, 1, 3, 5).reshape(B * P, K)
    ref_w = ref_dE.double().t() @ ref_patches.double()
    from tests import gemm_reference as GR
    # the outputs are ACCUMULATED into (+=): once into zeros, once into buffers that already hold values of the gradients' own size -- an overwrite fails the second
    for seeded in (False, True):
        s_pos = torch.randn(T, D, generator=g) * float(B) ** 0.5 if seeded else torch.zeros(T, D)
        s_cls = torch.randn(D, generator=g) * float(B) ** 0.5 if seeded else torch.zeros(D)
        s_w = torch.randn(D, K, generator=g) * float(ref_w.abs().mean()) if seeded else torch.zeros(D, K)
        dpos, dcls, gw = s_pos.to(DEV), s_cls.to(DEV), s_w.to(DEV)
        dE.zero_()
        ops.embed_bwd(dx.to(DEV), dpos, dcls, dE, B, T, Tp, D)
        autograd.patch_weight_grad(dE, patches, gw, D, K, B * P)
        torch.cuda.synchronize()
        # position / class sums: exact to the f32 rounding of a B-term sum (seeded: the value already there is one more term, B + 1 terms and B roundings)
        terms = x64[:, :T].abs().sum(0)
        tol = B * 2.0 ** -24 * (terms + s_pos.double().abs())
        err = (dpos.cpu().double() - (ref_pos + s_pos.double())).abs()
        print(f"embed_bwd B={B} grid={grid} p={p} seeded={seeded}: max |err| / tol, position = {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol).all())
        tol_c = B * 2.0 ** -24 * (terms[0] + s_cls.double().abs())
        assert bool(((dcls.cpu().double() - (ref_pos[0] + s_cls.double())).abs() <= tol_c).all())
        # the packed bf16 rows: RNE of the patch rows, nothing else
        assert torch.equal(dE[:B * P].cpu(), ref_dE) and not bool(dE[B * P:].any())
        assert bool((dE_all[ops.pad_rows(B * P):].view(torch.int16) == 0x4B5A).all())
        # weight gradient: bf16 operands (products exact in f32), f32 accumulation over B P terms in an order the test does not assume, plus the slab
        # reduction's adds (at most 256 splits) and the add into the value already there: |err| <= gamma2(B P + 257 [+ 1]) (sum |dE| |patches| + |seed|)
        # (tests/gemm_reference.py, any-order form)
        tol_w = GR.gamma2(B * P + 257 + seeded) * (ref_dE.double().abs().t() @ ref_patches.double().abs() + s_w.double().abs()) + 2.0 ** -126
        err_w = (gw.cpu().double() - (ref_w + s_w.double())).abs()
        print(f"   patch weight gradient [D={D}, K={K}] seeded={seeded}: max |err| / tol = {float((err_w / tol_w).max()):.3f}")
        assert bool((err_w <= tol_w).all())
    # im2row in the parameter's (c, i, j) order
    assert torch.equal(patches[:B * P, :K].cpu(), ref_patches) and not bool(patches[:, K:].any())


@pytest.mark.parametrize("B,T,D", [(1, 2, 8), (3, 257, 8)])      # the smallest problem (one thread); T D / 8 = 257 threads: the second workgroup owns one token
def test_embed_bwd_alone_at_the_edges_of_its_grid(B, T, D):
    """owl_embed_bwd alone: dpos / dcls against float64 with the B-term bound of the test above, dE the RNE of the patch rows; pad rows T .. Tp of dx are
    NaN, dE and dpos carry sentinel rows behind them."""
    P, Tp = T - 1, (T + 7) // 8 * 8
    g = torch.Generator().manual_seed(13 + T)
    dx = torch.randn(B, Tp, D, generator=g)
    dx[:, T:] = float("nan")
    s_pos, s_cls = torch.randn(T, D, generator=g), torch.randn(D, generator=g)
    dpos = torch.full((T + 2, D), 12345.678, device=DEV); dpos[:T] = s_pos.to(DEV)
    dcls = torch.full((2, D), 12345.678, device=DEV); dcls[0] = s_cls.to(DEV)
    dE = torch.full((B * P + 8, D), 0x4B5A, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    dx_dev = dx.to(DEV)
    ops.embed_bwd(dx_dev, dpos, dcls, dE, B, T, Tp, D)
    torch.cuda.synchronize()
    x64 = dx.double()
    ref = x64[:, :T].sum(0) + s_pos.double()
    tol = B * 2.0 ** -24 * (x64[:, :T].abs().sum(0) + s_pos.double().abs())
    assert bool(((dpos[:T].cpu().double() - ref).abs() <= tol).all())
    ref_c = x64[:, 0].sum(0) + s_cls.double()
    assert bool(((dcls[0].cpu().double() - ref_c).abs() <= B * 2.0 ** -24 * (x64[:, 0].abs().sum(0) + s_cls.double().abs())).all())
    assert torch.equal(dE[:B * P].cpu(), dx[:, 1:T].reshape(B * P, D).to(torch.bfloat16))
    assert bool((dE[B * P:].view(torch.int16) == 0x4B5A).all()) and bool((dpos[T:] == 12345.678).all()) and bool((dcls[1] == 12345.678).all())
    assert torch.equal(dx_dev[:, :T].cpu(), dx[:, :T]) and bool(torch.isnan(dx_dev[:, T:]).all())


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------------------------
def test_full_fine_tune_backward_is_bitwise_reproducible():
    cfg = get_config("tiny")
    Wnp, img, d_boxes, d_sims, _ = _reference("tiny", 5)
    out = []
    for _ in range(2):
        model = OwlViT(cfg, Wnp, DEV, trainable=EVERYTHING)
        pb, _, ps, _ = model(torch.from_numpy(img).to(DEV))
        torch.autograd.backward([pb, ps], [d_boxes.to(DEV), d_sims.to(DEV)])
        torch.cuda.synchronize()
        out.append(model.flat_grad.clone())
    assert torch.equal(out[0], out[1]) and float(out[0].abs().max()) > 0


# ---- 9. overlap tail with a low floor -----------------------------------------------------------------------------------------------------------
def test_deferred_tail_with_trainable_embeddings_is_bitwise_the_inline_schedule():
    """With trainable embeddings the next forward has no frozen prefix: it must wait for the tail before the patch embedding (and before it recasts the
    image the tail's backward still reads)."""
    def train(overlap, steps=3):
        cfg = get_config("tiny")
        model = OwlViT(cfg, weights.make_weights(cfg), DEV, trainable=EVERYTHING)
        labels, boxes = synth.make_targets(cfg, 4, max_boxes=5)
        lab = [torch.from_numpy(x).to(DEV) for x in labels]; box = [torch.from_numpy(x).to(DEV) for x in boxes]
        crit = PushPullLoss(cfg.n_classes, None)
        opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, overlap=overlap)
        assert model.overlap_tail == overlap
        g = torch.Generator(device="cpu").manual_seed(7)
        imgs = [torch.randn(4, 3, cfg.image_size, cfg.image_size, generator=g).to(DEV) for _ in range(steps)]
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
        return model.flat_param.clone(), torch.stack(hist).cpu()

    p0, h0 = train(False)
    p1, h1 = train(True)
    assert torch.equal(h0, h1) and torch.equal(p0, p1)
    assert bool(torch.isfinite(h0).all())


# ---- 10. errors --------------------------------------------------------------------------------------------------------------------------------
def test_construction_and_state_errors_on_the_device():
    cfg = get_config("tiny")
    Wnp = weights.make_weights(cfg)
    with pytest.raises(ValueError, match=r"part of the unit `backbone\.encoder\.layers\.11`.*layer_norm1\.weight"):
        OwlViT(cfg, Wnp, DEV, trainable=("layers.11.self_attn", "layers.11.mlp", "queries"))
    with pytest.raises(ValueError, match="selects no parameter"):
        OwlViT(cfg, Wnp, DEV, trainable=())
    model = OwlViT(cfg, Wnp, DEV, trainable=("queries", "class_predictor", "box"))
    img = torch.from_numpy(synth.make_images(cfg, 2)).to(DEV)
    model.p("backbone.post_layernorm.weight").requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"trainable set.*not supported.*trainable="):
        model(img)
    model.p("backbone.post_layernorm.weight").requires_grad_(False)
    model.p("queries").requires_grad_(False)
    with pytest.raises(RuntimeError, match="trainable set"):
        model(img)
    model.p("queries").requires_grad_(True)
    other = OwlViT(cfg, Wnp, DEV)
    sd = FusedAdamW(other).state_dict()
    with pytest.raises(ValueError, match="different trainable set"):
        FusedAdamW(model).load_state_dict(sd)
    opt = FusedAdamW(model)
    opt.load_state_dict(FusedAdamW(model).state_dict())          # its own set loads
