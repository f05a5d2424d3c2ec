"""-m gpu: a training step's bits do not depend on what the model did before it (profiles/history_independence.md).

probe(model, optimizer) is ONE fixed training step on images X and targets t -- forward, criterion, backward, optimizer.step(), then one no-grad forward --
and returns the bits of pred_boxes, the sims / logits, the losses, flat_grad, and after the step flat_param, the optimizer's m, v and EMA and the eval
outputs.  Per case a DIRTY model runs a prelude (other batches, other batch sizes, eval forwards and post-processing, a step that went NaN, the other
box-head backward, the deferred-tail schedule, the prefix cache); its state_dict() and the optimizer's are taken; a CLEAN model and optimizer are built
from them in the same process; the probe runs on both and every tensor must be bit-equal.  No tolerance anywhere.

Before the probe the invariants autograd.py documents are asserted on the dirty model so that a failure localises: du0z all zero, the pad columns of the
transposed weight-gradient operands zero, the compact operands' rows at and beyond cap_pad zero.  test_the_probe_sees_* are the controls: a 1.0 written
into such a buffer of the clean model changes the probe's flat_grad, and restoring the buffer restores the bits."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import autograd, ops  # noqa: E402
from owl_vit_object_detection_amd import preprocess as PP  # noqa: E402
from owl_vit_object_detection_amd import weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import OpenVocabLoss, PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.optim import FusedAdamW  # noqa: E402
from owl_vit_object_detection_amd.postprocess import PostProcess, SlicedPostProcess  # noqa: E402

DEV = "cuda"
NQ = 5
EVERYTHING = ("backbone", "post_post_layernorm", "class_predictor", "box_head", "queries")
# name -> (config, image size or None = native, trainable set, the probe's batch size, its targets per image, a batch with MORE matched rows, one with FEWER).
# The counts keep box_rows_cap_pad(B * max count) * 8 <= B * P, so that every step's box gradient takes the row path under box_backward = "auto".
MODELS = {
    "tiny": ("tiny", None, None, 3, (2, 1, 1), (2, 2, 2), (1, 1, 1)),
    "small": ("small", None, None, 2, (5, 3), (12, 9), (2, 1)),
    "tiny-full": ("tiny", 128, EVERYTHING, 3, (3, 1, 2), (6, 8, 7), (1, 1, 1)),          # full fine-tune at 128: _pre_ws, dU, the patch-embedding dW
    "tiny-l14": ("tiny-l14", None, None, 3, (2, 1, 1), (2, 2, 2), (1, 1, 1)),            # frozen layers ABOVE the trainable one: the dX-only chain
    "tiny-head": ("tiny", None, None, 3, (2, 1, 1), (2, 2, 2), (1, 1, 1)),               # OpenVocabLoss with a TRAINABLE logit head: ovb_rowgrad, the head-gradient workspace
}
_ctx = {}


class Ctx:
    def __init__(self, name, kind):
        cname, size, self.trainable, self.B, self.counts, self.more, self.fewer = MODELS[name]
        cfg0 = get_config(cname)
        self.cfg = cfg0 if size is None else cfg0.replace(image_size=size, pos_grid=cfg0.grid)
        self.W = weights.make_weights(cfg0)
        self.kind, self.train_head = kind, name.endswith("-head")
        g = torch.Generator().manual_seed(22)
        q = torch.randn(8, NQ, self.cfg.text_dim, generator=g)
        self.q = (q / q.norm(dim=-1, keepdim=True)).to(DEV)
        D = self.cfg.hidden
        self.head = {"logit_shift.weight": 0.3 / D ** 0.5 * torch.randn(D, generator=g), "logit_shift.bias": torch.tensor([0.05]),
                     "logit_scale.weight": 1.0 / D ** 0.5 * torch.randn(D, generator=g), "logit_scale.bias": torch.tensor([0.1])}
        self.crit = PushPullLoss(self.cfg.n_classes, None) if kind == "pushpull" else OpenVocabLoss()

    def model(self, state=None):
        m = OwlViT(self.cfg, self.W if state is None else state, DEV, trainable=self.trainable)
        if self.kind == "openvocab":
            m.set_logit_head(self.head, trainable=self.train_head)          # (its four leaves get gradients; nothing here steps them)
        return m

    def optimizer(self, model, overlap=False):
        return FusedAdamW(model, lr=1e-3, weight_decay=0.1, max_norm=1.0, ema_decay=0.99, overlap=overlap)

    def images(self, B, seed):
        H, W = self.cfg.image_hw
        return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)

    def targets(self, counts, seed):
        """Per image `n` boxes inside the image and labels of the criterion's range (a class of the bank / an index into the image's query list)."""
        rs = np.random.RandomState(seed)
        labels, boxes = [], []
        for n in counts:
            xy, wh = rs.rand(n, 2) * 0.6, 0.02 + rs.rand(n, 2) * 0.35
            boxes.append(torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32)).to(DEV))
            labels.append(torch.from_numpy(rs.randint(0, self.cfg.n_classes if self.kind == "pushpull" else NQ, n).astype(np.int64)).to(DEV))
        return labels, boxes

    def batch(self, counts, seed):
        return self.images(len(counts), seed), self.targets(counts, seed + 1)


def ctx(name, kind):
    if (name, kind) not in _ctx:
        _ctx[(name, kind)] = Ctx(name, kind)
    return _ctx[(name, kind)]


# ---- one step ---------------------------------------------------------------------------------------------------------------------------------
def forward(c, model, img, ids=None):
    if c.kind == "pushpull":
        pb, _, cl, _ = model(img) if ids is None else model(img, image_ids=ids)
        return pb, cl
    return model.forward_queries(img, c.q[:img.shape[0]])


def eval_forward(c, model, img):
    with torch.no_grad():
        if c.kind == "pushpull":
            pb, _, cl, _ = model(img)
            return pb, cl
        return model.detect(img, c.q[:img.shape[0]])


def losses(c, pb, cl, tg):
    labels, boxes = tg
    if c.kind == "pushpull":
        return c.crit(cl, labels, pb, boxes)
    return c.crit(cl, pb, [{"class_labels": l, "boxes": b} for l, b in zip(labels, boxes)])


def zero_head_grads(model):
    for p in model.logit_head_parameters() if model.logit_head is not None else []:
        p.grad = None


def train_step(c, model, opt, img, tg, ids=None):
    opt.zero_grad()
    zero_head_grads(model)
    pb, cl = forward(c, model, img, ids)
    sum(losses(c, pb, cl, tg).values()).backward()
    opt.step()


def probe(c, model, opt, ids=None, path="rows"):
    """The fixed step.  Everything it returns is a clone taken behind a synchronisation."""
    img, tg = c.batch(c.counts, 100)
    opt.zero_grad()
    zero_head_grads(model)
    model.last_box_backward = None
    pb, cl = forward(c, model, img, ids)
    l = losses(c, pb, cl, tg)
    sum(l.values()).backward()
    model.finish()
    torch.cuda.synchronize()
    assert model.last_box_backward == path, model.last_box_backward
    out = dict(pred_boxes=pb.detach().clone(), cls=cl.detach().clone(), flat_grad=model.flat_grad.clone(), **{k: v.detach().clone() for k, v in l.items()})
    if c.train_head:
        out.update({f"head_grad_{i}": p.grad.detach().clone() for i, p in enumerate(model.logit_head_parameters())})
        assert len(model.logit_head_parameters()) == 4 and all(float(out[f"head_grad_{i}"].abs().max()) > 0 for i in range(4))
    opt.step()
    model.finish()
    torch.cuda.synchronize()
    out.update(flat_param=model.flat_param.detach().clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(), ema=opt.ema.clone(),
               grad_norm=opt.last_grad_norm.clone())
    eb, ec = eval_forward(c, model, img)
    torch.cuda.synchronize()
    out.update(eval_boxes=eb.clone(), eval_cls=ec.clone())
    return out


def snapshot(model, opt):
    model.finish()
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    osd = {k: (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in opt.state_dict().items()}
    return sd, osd


def restore(model, opt, sd, osd):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    opt.load_state_dict(osd)


def same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.shape == y.shape and torch.equal(x.view(-1).view(torch.uint8), y.view(-1).view(torch.uint8)), f"{what}: {k} differs"
    assert bool(torch.isfinite(a["flat_grad"]).all()) and bool(torch.isfinite(a["flat_param"]).all()), what
    assert float(a["flat_grad"].abs().max()) > 0


def assert_invariants(c, model, B, rows_ran):
    """What autograd.py promises about the buffers that outlive a backward, at batch size B.  The buffers must BE there -- a renamed key or an evicted size
    would otherwise turn this into nothing: every prelude's last step trains at B, and rows_ran says whether a row-path backward has run at B since the
    workspaces were made."""
    assert ("bwd", B) in model._ws, sorted(map(str, model._ws))
    bw, cfg = model._ws[("bwd", B)], c.cfg
    for key, rows in (("tA", B * cfg.tokens_padded), ("tB", B * cfg.tokens_padded), ("tAh", B * cfg.patches), ("tBh", B * cfg.patches)):
        t = bw[key]
        assert (t is None) == (key in ("tA", "tB") and bool(bw["tn_all"])), key          # (no token-row pair where every token-row product is on the TN kernel)
        if t is not None:
            assert t.shape[1] == ops.pad_rows(rows) and t.shape[1] > rows
            assert bool((t[:, rows:].view(torch.int16) == 0).all()), f"pad columns of {key} are dirty"
    assert ("box_rows" in bw) == rows_ran
    if rows_ran:
        rw = bw["box_rows"]
        assert (rw["du0z"] is not None) == ("box_head" in model._units)
        if rw["du0z"] is not None:
            assert rw["du0z"].shape[0] >= B * cfg.patches and bool((rw["du0z"].view(torch.int16) == 0).all()), "du0z is not all zero between backwards"
        for key in ("du1c", "du0c", "ub0c", "dfc"):
            t = rw[key][rw["cap_pad"]:]
            assert t.shape[0] > 0 and bool((t.view(torch.int32 if t.dtype == torch.float32 else torch.int16) == 0).all()), f"{key}: rows at and beyond cap_pad are dirty"


# ---- the preludes: each returns the keyword arguments of the probe ------------------------------------------------------------------------------------
def other_batches(c, model, opt):
    train_step(c, model, opt, *c.batch(c.more, 200))          # more matched rows than the probe's: the listed rows shrink and move afterwards
    train_step(c, model, opt, *c.batch(c.fewer, 210))
    if c.kind == "openvocab":                                   # (PushPullLoss, like the reference, takes no image without targets)
        train_step(c, model, opt, *c.batch((0,) + tuple(c.more[1:]), 220))
        train_step(c, model, opt, *c.batch((0,) * c.B, 230))
    return {}


def other_batch_sizes(c, model, opt):
    # B -> another -> 5 -> B: 5 evicts a cached size (two are kept) and splits unevenly over the two encoder streams; the probe then runs at B
    for i, B in enumerate((c.B, 2 if c.B == 3 else 3, 5, c.B)):
        train_step(c, model, opt, *c.batch((1,) * B, 300 + 10 * i))
    return {}


def eval_between(c, model, opt):
    train_step(c, model, opt, *c.batch(c.fewer, 400))
    S = c.cfg.image_size
    for B in (c.B, c.B + 1):
        pb, cl = eval_forward(c, model, c.images(B, 410 + B))
        PostProcess(0.0, 0.3)(pb, cl)
        PostProcess(0.0, 0.3, nms_route="per_class")(pb, cl, top_k=7)
    proc = PP.DeviceImageProcessor(S, device=DEV)
    src = np.random.RandomState(7).randint(0, 256, (int(1.6 * S), int(2.2 * S), 3)).astype(np.uint8)
    pix, plan = proc.slices([src], slice_size=S)
    assert pix.shape[0] > c.B + 1          # one more batch size, eval only
    pb, cl = eval_forward(c, model, pix)
    SlicedPostProcess(0.0, 0.3, per_slice_top_k=20)(pb, cl, plan)
    train_step(c, model, opt, *c.batch(c.more, 420))
    return {}


def nan_then_clean(c, model, opt):
    """One step whose box gradient breaks the row path's promise (more non-zero rows than marked): NaN in the gradients, then in the parameters and the
    moments.  Then zero_grad, the state from before it, and the probe."""
    train_step(c, model, opt, *c.batch(c.fewer, 500))
    sd, osd = snapshot(model, opt)
    img, tg = c.batch(c.more, 510)
    opt.zero_grad()
    zero_head_grads(model)
    pb, cl = forward(c, model, img)
    p2, c2 = pb.detach().clone().requires_grad_(True), cl.detach().clone().requires_grad_(True)
    sum(losses(c, p2, c2, tg).values()).backward()
    assert int((p2.grad.reshape(-1, 4) != 0).any(dim=1).sum()) > 1
    torch.autograd.backward([pb, cl], [autograd.mark_box_rows(p2.grad.clone(), 1), c2.grad])
    model.finish()
    torch.cuda.synchronize()
    assert model.last_box_backward == "rows" and bool(torch.isnan(model.p("box_head.dense0.weight").grad).any())
    assert model._ws[("bwd", c.B)]["box_rows"]["count_flag"][:2].tolist() == [1, 1]
    opt.step()
    model.finish()
    assert bool(torch.isnan(model.flat_param).any())
    opt.zero_grad()
    restore(model, opt, sd, osd)
    return dict(check_flag=True)


def dense_then_rows(c, model, opt):
    model.box_backward = "dense"
    train_step(c, model, opt, *c.batch(c.more, 600))
    train_step(c, model, opt, *c.batch(c.fewer, 610))
    assert model.last_box_backward == "dense"
    model.box_backward = "auto"
    return {}


def rows_then_dense(c, model, opt):
    train_step(c, model, opt, *c.batch(c.more, 620))
    train_step(c, model, opt, *c.batch(c.fewer, 630))
    assert model.last_box_backward == "rows"
    return dict(path="dense")


def schedules(c, model, opt):
    """(the dirty model runs the deferred tail with pre-transposed weights: run_case builds it so)  Two steps, the snapshot -- which has to wait for the
    tail --, then `pre_step`: one more step that BOTH models take (the clean one in line), so that the dirty probe follows an optimizer step at once: the
    one-shot bf16 token is live and nothing has waited for the tail stream."""
    assert model.overlap_tail and model.pretranspose
    for i, counts in enumerate((c.more, c.fewer)):
        train_step(c, model, opt, *c.batch(counts, 700 + 10 * i))
    return dict(pre_step=c.batch(c.counts, 720))


def prefix_cache(c, model, opt):
    """Capacity B + 1: B other ids fill all but one slot, ONE of the probe's images still gets a slot (first come, first kept; nothing is evicted), an eval
    forward with unseen ids finds the cache full, and the probe then mixes that one kept image with B - 1 computed ones.  The clean model has no cache."""
    cache = model.enable_prefix_cache(max_images=c.B + 1)
    train_step(c, model, opt, *c.batch(c.fewer, 800), ids=list(range(10, 10 + c.B)))
    img, tg = c.batch(c.counts, 100)
    train_step(c, model, opt, img, c.targets(c.more, 811), ids=list(range(c.B)))
    with torch.no_grad():
        model(c.images(c.B, 820), image_ids=list(range(20, 20 + c.B)))
    kept = [bool(k) for k in cache.contains(list(range(c.B)))]
    assert len(cache) == c.B + 1 and sum(kept) == 1, (len(cache), kept)          # the probe mixes a kept image with computed ones
    return dict(ids=list(range(c.B)))


PRELUDES = dict(other_batches=other_batches, other_batch_sizes=other_batch_sizes, eval_between=eval_between, nan_then_clean=nan_then_clean,
                dense_then_rows=dense_then_rows, rows_then_dense=rows_then_dense, schedules=schedules, prefix_cache=prefix_cache)


def run_case(name, kind, prelude):
    c = ctx(name, kind)
    dirty = c.model()
    if prelude == "schedules":
        dirty.pretranspose = True
    dopt = c.optimizer(dirty, overlap=prelude == "schedules")
    kw = PRELUDES[prelude](c, dirty, dopt)
    check_flag, ids, path = kw.get("check_flag", False), kw.get("ids"), kw.get("path", "rows")
    sd, osd = snapshot(dirty, dopt)
    clean = c.model(sd)
    copt = c.optimizer(clean)
    copt.load_state_dict(osd)
    assert torch.equal(clean.flat_param, dirty.flat_param) and torch.equal(copt.ema, dopt.ema) and copt.step_count == dopt.step_count
    assert_invariants(c, dirty, c.B, rows_ran=prelude != "dense_then_rows")
    if path == "dense":
        dirty.box_backward = clean.box_backward = "dense"
    pre = kw.get("pre_step")
    if pre is not None:
        train_step(c, clean, copt, *pre)
        clean.finish()
        torch.cuda.synchronize()
    want = probe(c, clean, copt, path=path)
    if pre is not None:
        train_step(c, dirty, dopt, *pre)
        assert dirty._bf16_current and dirty._param_event is not None          # the token is live, the tail has not been waited for
    got = probe(c, dirty, dopt, ids=ids, path=path)
    same(got, want, f"{name} {kind} after {prelude}")
    assert_invariants(c, dirty, c.B, rows_ran=True)
    if check_flag:
        assert dirty._ws[("bwd", c.B)]["box_rows"]["count_flag"][1].item() == 0, "the overflow flag outlived the step that set it"


def _cases():
    out = []
    for name in ("tiny", "small"):
        for kind in ("pushpull", "openvocab"):
            out += [(name, kind, p) for p in PRELUDES if not (p == "prefix_cache" and kind == "openvocab")]          # (forward_queries takes no image ids)
    out += [("tiny-full", "pushpull", p) for p in PRELUDES if p != "prefix_cache"]                                  # (no frozen prefix to cache)
    out += [("tiny-full", "openvocab", "other_batches"), ("tiny-full", "openvocab", "other_batch_sizes")]
    out += [("tiny-l14", "pushpull", "other_batch_sizes")]
    out += [("tiny-head", "openvocab", p) for p in ("other_batches", "other_batch_sizes", "nan_then_clean")]
    return out


@pytest.mark.parametrize("name,kind,prelude", _cases(), ids=lambda v: str(v))
def test_probe_after_a_prelude_equals_the_probe_on_a_fresh_model(name, kind, prelude):
    run_case(name, kind, prelude)


# ---- controls: the probe sees the buffers the invariants are about --------------------------------------------------------------------------------
def _control(name, dirty_it):
    """probe; dirty one buffer of the same model, the state put back, probe: flat_grad differs; restore the buffer, the state put back, probe: the first bits."""
    c = ctx(name, "pushpull")
    model = c.model()
    opt = c.optimizer(model)
    train_step(c, model, opt, *c.batch(c.fewer, 900))          # (makes the backward workspaces of this batch size)
    sd, osd = snapshot(model, opt)
    base = probe(c, model, opt)
    restore(model, opt, sd, osd)
    same(probe(c, model, opt), base, "the state put back")
    restore(model, opt, sd, osd)
    undo = dirty_it(c, model._ws[("bwd", c.B)])
    seen = probe(c, model, opt)
    assert not torch.equal(seen["flat_grad"], base["flat_grad"]), "the probe does not see this buffer"
    undo()
    restore(model, opt, sd, osd)
    same(probe(c, model, opt), base, "the buffer restored")


def test_the_probe_sees_du0z():
    def dirty_it(c, bw):
        rw = bw["box_rows"]
        listed = set(rw["row_list"][:int(rw["count_flag"][0])].tolist())
        row = next(r for r in range(c.B * c.cfg.patches) if r not in listed)          # (the list of the probe that has just run: the same state, the same matches)
        rw["du0z"][row, 3] = 1.0

        def undo():
            rw["du0z"][row, 3] = 0.0
        return undo
    _control("tiny", dirty_it)


def test_the_probe_sees_the_pad_columns_of_the_transposed_operands():
    """box_head.dense0's weight gradient at `tiny` widths runs on the NT route: dy^T in tAh, x^T in tBh, contracted over pad_rows(B * P) columns.  A pad
    column adds tAh[i, k] * tBh[j, k] to dW[i, j], so the value goes into the SAME pad column of both operands (one element each): either alone is
    multiplied by the other's zero."""
    def dirty_it(c, bw):
        k = c.B * c.cfg.patches          # the first pad column
        assert k < bw["tAh"].shape[1] and not autograd._dw_plan(c.cfg.hidden, c.cfg.hidden, bias=True, tn_all=bw["tn_all"], rows=k).tn
        bw["tAh"][1, k] = 1.0
        bw["tBh"][2, k] = 1.0

        def undo():
            bw["tAh"][1, k] = 0.0
            bw["tBh"][2, k] = 0.0
        return undo
    _control("tiny", dirty_it)
