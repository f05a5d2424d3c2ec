"""-m gpu: the box head's backward on the rows that carry a gradient (csrc/box_rows_bwd.hip, autograd.backward_impl's row path).

Kernel cases: the compaction against tests/box_rows_reference.compact on its edge cases; gather, put and scatter-add bit for bit against the rows of the
dense kernels' operands and results.  Model cases: `box_backward="auto"` against `"dense"` from the same state through PushPullLoss and OpenVocabLoss:
the WHOLE gradient bucket bitwise equal (the row path keeps the dense launches' grouping and order of every sum), and the six box_head.* gradients inside
the bounds derived in tests/box_rows_reference.py.  Every case prints its worst err / tol; profiles/box_rows_bwd.md records them.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import box_rows_reference as R  # noqa: E402
from tests.gemm_reference import check  # noqa: E402
from owl_vit_object_detection_amd import _lib, autograd, ops, synth, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config  # noqa: E402
from owl_vit_object_detection_amd.losses import OpenVocabLoss, PushPullLoss  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402

DEV = "cuda"
CAP = 8
bf = torch.bfloat16


# ---- kernel cases -------------------------------------------------------------------------------------------------------------------------
def _compact_dev(db, cap=CAP):
    rl = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    cf = torch.full((ops.box_rows_state_ints(db.shape[0]),), -7, dtype=torch.int32, device=DEV)
    ops.box_rows_compact(db.to(DEV).contiguous(), db.shape[0], cap, rl, cf)
    torch.cuda.synchronize()
    return rl, cf


def _compact_cases(rows):
    nan = float("nan")
    cases = [("none", [], None), ("first", [0], None), ("last", [rows - 1], None), ("nan_row", [], {3: [0.0, nan, 0.0, 0.0]}),
             ("neg_zero_only", [1], {4: [-0.0, -0.0, -0.0, -0.0]}), ("fourth_component", [], {5: [0.0, 0.0, 0.0, 1e-30]})]
    if rows >= CAP + 1:
        step = rows // (CAP + 1)
        exact = [i * step for i in range(CAP)]
        cases += [("exactly_cap", exact, None), ("cap_plus_1", exact + [rows - 1], None)]
    else:          # fewer rows than cap: every row listed is the fullest list there is
        cases += [("all_rows", list(range(rows)), None)]
    if rows > 2048:          # more than one workgroup of the compaction (1024 rows each): both sides of every boundary, the ragged last one
        cases += [("across_workgroups", [1023, 1024, 2047, 2048, rows - 1], None), ("second_workgroup_only", [1500], None)]
    return cases


@pytest.mark.parametrize("rows", [7, 64, 577, 2500])
def test_compaction_edge_cases(rows):
    for name, listed, special in _compact_cases(rows):
        db = R.make_case(rows, 8, listed, special=special)["dboxes"]
        want, n, over = R.compact(db.numpy(), CAP)
        rl, cf = _compact_dev(db)
        assert cf[:2].tolist() == [n, int(over)], (name, cf.tolist(), n, over)
        assert rl[:n].tolist() == want.tolist(), (name, rl.tolist(), want.tolist())
        assert over == (name == "cap_plus_1")
        rl2, cf2 = _compact_dev(db)
        assert torch.equal(rl, rl2) and torch.equal(cf, cf2), name          # deterministic


def _dense_tail(c, rows, D):
    """The dense kernel on the same inputs: du1 bf16 [rows, D], (dW2 | db2) f32, colsum f32."""
    du1 = torch.zeros(ops.pad_rows(rows), D, dtype=bf, device=DEV)
    part = torch.full((_lib.load().owl_box_final_bwd_blocks(rows), 5 * D + 4), float("nan"), device=DEV)          # scratch: NaN, so a word read before it is written shows
    g, cs = torch.zeros(4 * D + 4, device=DEV), torch.zeros(D, device=DEV)
    ops.box_final_bwd(c["dboxes"], c["sig"], c["hb1"], c["ub1"], c["w2"], du1, part, g, rows, D, du1_colsum=cs)
    return du1, g, cs


def _case_dev(rows, D, listed, special=None):
    c = R.make_case(rows, D, listed, special=special)
    d = {k: v.to(DEV) for k, v in c.items()}
    for k in ("hb1", "ub1", "hb0", "ub0", "feats", "w1"):
        d[k] = d[k].to(bf).contiguous()
    return c, d


@pytest.mark.parametrize("count", [0, 1, CAP])
@pytest.mark.parametrize("D,rows", [(64, 577), (768, 577), (64, 2500)])          # 577 rows: 73 dense workgroups, the serial reduce; 2500: 313, the tall one
def test_tail_gather_scatter_against_the_reference_and_the_dense_kernels(D, rows, count):
    cap_pad = ops.box_rows_cap_pad(CAP)
    # eight rows: three in one dense group of 8 (8, 9, 15), its neighbour (16), two in a far group, and both sides of the last (ragged) group's edge
    listed = {0: [], 1: [76], CAP: [8, 9, 15, 16, 300, 301, rows - 2, rows - 1]}[count]
    assert len(listed) == count
    c, d = _case_dev(rows, D, listed)
    want, n, over = R.compact(c["dboxes"].numpy(), CAP)
    rl, cf = _compact_dev(c["dboxes"])
    assert n == count and not over and rl[:n].tolist() == want.tolist() == listed
    idx = torch.as_tensor(listed, dtype=torch.int64, device=DEV)
    # ---- the dense tail's du1, and its listed rows gathered: bits of the rows, exact zeros up to cap_pad, sentinel rows beyond cap_pad stay
    alloc = ops.pad_rows(cap_pad)
    du1_d, _, _ = _dense_tail(d, rows, D)
    du1c = torch.full((alloc, D), 3.0, dtype=bf, device=DEV)
    ops.box_rows_gather([(du1_d, du1c)], rl, cf, rows, cap_pad, D)
    torch.cuda.synchronize()
    assert torch.equal(du1c[:n].view(torch.int16), du1_d[idx].view(torch.int16))
    assert bool((du1c[n:cap_pad].view(torch.int16) == 0).all()) and bool((du1c[cap_pad:] == 3.0).all())
    keep = torch.ones(du1_d.shape[0], dtype=torch.bool, device=DEV)
    keep[idx] = False
    assert bool((du1_d[keep].view(torch.int16) & 0x7fff == 0).all())          # every other row of the dense du1 is +-0: the list loses nothing
    # put / clear: the listed rows where they lie in a zero buffer, and zero again
    z0, z1 = torch.zeros_like(du1_d), torch.zeros_like(du1_d)
    ops.box_rows_put([(du1c, z0)], rl, cf, rows, CAP, D)
    ops.box_rows_put([(du1c, z0), (du1c, z1)], rl, cf, rows, CAP, D)
    torch.cuda.synchronize()
    for z in (z0, z1):
        assert torch.equal(z[idx].view(torch.int16), du1_d[idx].view(torch.int16)) and bool((z[keep].view(torch.int16) == 0).all())
    ops.box_rows_put([(None, z0), (None, z1)], rl, cf, rows, CAP, D)
    torch.cuda.synchronize()
    assert bool((z0.view(torch.int16) == 0).all()) and bool((z1.view(torch.int16) == 0).all())
    # ---- gather: three sources in one launch; bits of the listed rows, zero rows up to cap_pad, nothing beyond
    dst = [torch.full((alloc, D), 3.0, dtype=bf, device=DEV) for _ in range(3)]
    ops.box_rows_gather([(d["hb0"], dst[0]), (d["ub0"], dst[1]), (d["feats"], dst[2])], rl, cf, rows, cap_pad, D)
    one = torch.full((alloc, D), 3.0, dtype=bf, device=DEV)
    ops.box_rows_gather([None, (d["ub0"], one), None], rl, cf, rows, cap_pad, D)          # (a frozen box head gathers ub0 alone)
    torch.cuda.synchronize()
    for src, t in ((d["hb0"], dst[0]), (d["ub0"], dst[1]), (d["feats"], dst[2]), (d["ub0"], one)):
        assert torch.equal(t[:n].view(torch.int16), src[idx].view(torch.int16))
        assert bool((t[n:cap_pad].view(torch.int16) == 0).all()) and bool((t[cap_pad:] == 3.0).all())
    # ---- the compact dX product + scatter-add against dfeats + the dense product, bit for bit
    du0c = torch.zeros(alloc, D, dtype=bf, device=DEV)
    ops.gemm(ops.EPI_DGELU_BF16, du1c.clone().index_fill_(0, torch.arange(cap_pad, alloc, device=DEV), 0.0), d["w1"].t().contiguous(), du0c, aux=dst[1], M=cap_pad, N=D, K=D)
    du0 = torch.zeros(ops.pad_rows(rows), D, dtype=bf, device=DEV)
    ops.gemm(ops.EPI_DGELU_BF16, du1_d, d["w1"].t().contiguous(), du0, aux=d["ub0"], M=rows, N=D, K=D)
    torch.cuda.synchronize()
    assert torch.equal(du0c[:n].view(torch.int16), du0[idx].view(torch.int16))
    gen = torch.Generator().manual_seed(3)
    w0T = (torch.randn(D, D, generator=gen) / D ** 0.5).to(DEV).to(bf)
    base = torch.randn(ops.pad_rows(rows), D, generator=gen).to(DEV)
    dense = base.clone()
    ops.gemm(ops.EPI_ACC_F32, du0, w0T, dense, M=rows, N=D, K=D)
    dfc = torch.full((alloc, D), float("nan"), device=DEV)
    ops.gemm(ops.EPI_F32, du0c, w0T, dfc, M=cap_pad, N=D, K=D)
    mine = base.clone()
    ops.box_rows_scatter_add(dfc, mine, rl, cf, rows, CAP, D)
    torch.cuda.synchronize()
    assert torch.equal(mine.view(torch.int32), dense.view(torch.int32))


def test_overflow_flag_becomes_nan_downstream():
    rows, D, cap_pad = 64, 64, 8
    listed = list(range(0, 63, 7))[:CAP] + [63]          # cap + 1 rows
    c, d = _case_dev(rows, D, listed)
    rl, cf = _compact_dev(c["dboxes"])
    assert cf[:2].tolist() == [CAP, 1]
    out = torch.zeros(ops.pad_rows(cap_pad), D, dtype=bf, device=DEV)
    ops.box_rows_gather([(d["ub0"], out)], rl, cf, rows, cap_pad, D)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:CAP].float()).all()) and bool((out[cap_pad:].view(torch.int16) == 0).all())


# ---- model cases --------------------------------------------------------------------------------------------------------------------------
NQ = 5
FROZEN_BOX = ("layers.11.", "queries")                       # the chain crosses a frozen box head (tests/test_trainable_sets_gpu.py)
HEADS_ONLY = ("queries", "class_predictor", "box")           # floor "heads": no d(feats)
BOX = "box_head."
_state = {}


def _inputs(cname, B):
    """Weights, images and targets of one shape, made once and left unchanged.  Targets per image are kept small enough for cap_pad * 8 <= B * P."""
    if (cname, B) not in _state:
        cfg = get_config(cname)
        nmax = max(1, min(16, (B * cfg.patches // 8) // 8 * 8 // B))
        labels, boxes = synth.make_targets(cfg, B, max_boxes=nmax)
        g = torch.Generator().manual_seed(22)
        q = torch.randn(B, NQ, cfg.text_dim, generator=g)
        D = cfg.hidden
        head = {"logit_shift.weight": 0.3 / D ** 0.5 * torch.randn(D, generator=g), "logit_shift.bias": torch.tensor([0.05]),
                "logit_scale.weight": 1.0 / D ** 0.5 * torch.randn(D, generator=g), "logit_scale.bias": torch.tensor([0.1])}
        _state[(cname, B)] = dict(cfg=cfg, W=weights.make_weights(cfg), img=torch.from_numpy(synth.make_images(cfg, B)), labels=labels, boxes=boxes,
                                  scales=synth.class_scales(cfg, labels), q=q / q.norm(dim=-1, keepdim=True), head=head)
    return _state[(cname, B)]


def _targets(s, B, empty):
    """empty: () | (b,) one image without targets | "all"."""
    labels = [torch.from_numpy(l).to(DEV) for l in s["labels"]]
    boxes = [torch.from_numpy(b).to(DEV) for b in s["boxes"]]
    for b in (range(B) if empty == "all" else empty):
        labels[b], boxes[b] = labels[b][:0], boxes[b][:0]
    return labels, boxes


def _loss(model, s, B, kind, empty, detached=None):
    """One gradient-recording forward + criterion -> (the summed loss, pred_boxes, the class output).  detached: leaves to run the criterion on instead."""
    labels, boxes = _targets(s, B, empty)
    img = s["img"].to(DEV)
    if kind == "pushpull":
        pb, _, cl, _ = model(img)
        crit = PushPullLoss(s["cfg"].n_classes, s["scales"])
        run = lambda p, c: sum(crit(c, labels, p, boxes).values())
    else:
        pb, cl = model.forward_queries(img, s["q"].to(DEV))
        crit = OpenVocabLoss()
        tg = [{"class_labels": l % NQ, "boxes": b} for l, b in zip(labels, boxes)]
        run = lambda p, c: sum(crit(c, p, tg).values())
    return run, pb, cl


def _backward(model, s, B, kind, empty, mode, upstream=None):
    """-> dict(fg, path, loss, pb): flat_grad after one backward from a zeroed bucket under model.box_backward = mode.  upstream: None (the criterion's own
    backward) or "unmarked" (the criterion's gradients recomputed on detached leaves and handed over times 1.0: the same values without the mark)."""
    model.box_backward = mode
    model.last_box_backward = None
    model.finish()
    model.flat_grad.zero_()
    run, pb, cl = _loss(model, s, B, kind, empty)
    if upstream is None:
        loss = run(pb, cl)
        loss.backward()
    else:
        p2, c2 = pb.detach().clone().requires_grad_(True), cl.detach().clone().requires_grad_(True)
        loss = run(p2, c2)
        loss.backward()
        torch.autograd.backward([pb, cl], [p2.grad * 1.0, c2.grad * 1.0])
    model.finish()
    torch.cuda.synchronize()
    return dict(fg=model.flat_grad.clone(), path=model.last_box_backward, loss=loss.detach().clone(), pb=pb.detach().clone())


def _dboxes(model, s, B, kind, empty):
    run, pb, cl = _loss(model, s, B, kind, empty)
    p2, c2 = pb.detach().clone().requires_grad_(True), cl.detach().clone().requires_grad_(True)
    run(p2, c2).backward()
    return p2.grad.detach().reshape(-1, 4).contiguous()


def _box_mask(model):
    m = torch.zeros(model.flat_grad.numel(), dtype=torch.bool, device=DEV)
    for n, off in model.flat_offsets.items():
        if n.startswith(BOX):
            m[off: off + model.p(n).numel()] = True
    return m


def _model(s, kind, **kw):
    model = OwlViT(s["cfg"], s["W"], DEV, **kw)
    if kind == "openvocab":
        model.set_logit_head(s["head"])
    return model


def _check_case(cname, B, kind, empty=(), tag="", **kw):
    s = _inputs(cname, B)
    cfg = s["cfg"]
    model = _model(s, kind, **kw)
    Mh, D = B * cfg.patches, cfg.hidden
    dense = _backward(model, s, B, kind, empty, "dense")
    bw = model._ws[("bwd", B)]
    t_box = "box_head" in model._units
    du_dense = (bw["du1"][:Mh].clone(), bw["du0"][:Mh].clone())
    rows1 = _backward(model, s, B, kind, empty, "auto")
    rows2 = _backward(model, s, B, kind, empty, "auto")
    assert dense["path"] == "dense" and rows1["path"] == "rows" and rows2["path"] == "rows"
    assert torch.equal(rows1["fg"].view(torch.int32), rows2["fg"].view(torch.int32))          # two runs of the row path: the same bits
    assert torch.equal(dense["loss"], rows1["loss"]) and torch.equal(dense["pb"], rows1["pb"])
    box = _box_mask(model)
    assert torch.equal(dense["fg"][~box].view(torch.int32), rows1["fg"][~box].view(torch.int32))          # everything outside box_head.*: bitwise
    assert torch.equal(dense["fg"].view(torch.int32), rows1["fg"].view(torch.int32))          # ... and box_head.* too: the dense launches' grouping and order
    assert bool(torch.isfinite(rows1["fg"]).all())
    # the listed rows' du1 / du0 are the dense launches' bits
    rw = bw["box_rows"]
    db = _dboxes(model, s, B, kind, empty)
    want, n, over = R.compact(db.cpu().numpy(), rw["cap_pad"])
    assert rw["count_flag"][:2].tolist() == [n, 0] and not over and rw["row_list"][:n].tolist() == want.tolist()
    idx = torch.as_tensor(want.astype(np.int64), device=DEV)
    assert torch.equal(rw["du1c"][:n].view(torch.int16), du_dense[0][idx].view(torch.int16))
    assert torch.equal(rw["du0c"][:n].view(torch.int16), du_dense[1][idx].view(torch.int16))
    if empty != "all":
        assert n >= 1
    if not t_box:
        assert not bool(box.any())
        return
    # the six sums against float64 on the operands the products read, each path inside the bound of its own chains
    ws = model._workspace(B)
    x = R.exact_six(db, ws["sig"][:Mh], ws["hb1"][:Mh], ws["ub1"][:Mh], ws["hb0"][:Mh], ws["ub0"][:Mh], ws["feats"][:Mh],
                    model.p("box_head.dense2.weight").detach(), None, want, given_du1=rw["du1c"][:n], given_du0=rw["du0c"][:n])
    cap_pad = rw["cap_pad"]
    assert bool((rw["du0z"].view(torch.int16) == 0).all())          # the dense operand of dense0's weight-gradient product is all zero again
    tol_d = R.bounds_six(x, Mh)
    worst = {}
    for name, fg, tol in (("rows", rows1["fg"], tol_d), ("dense", dense["fg"], tol_d)):
        w = 0.0
        for k in R.SIX:
            n_ = BOX + k
            off, p = model.flat_offsets[n_], model.p(n_)
            got = fg[off: off + p.numel()].view(p.shape)
            w = max(w, check(f"{name} {n_}", got, x["grads"][k], tol[k]))
        worst[name] = w
    print(f"[box rows {cname} B={B} {kind} {tag}] listed {n} of {Mh} rows (cap_pad {cap_pad}); worst err / bound against float64: rows {worst['rows']:.3f}, dense {worst['dense']:.3f}")


@pytest.mark.parametrize("kind", ["pushpull", "openvocab"])
@pytest.mark.parametrize("cname,B", [("tiny", 2), ("tiny", 3), ("small", 2), ("small", 3)])
def test_rows_path_matches_dense(cname, B, kind):
    _check_case(cname, B, kind)


@pytest.mark.parametrize("cname,B", [("tiny", 2), ("small", 3)])
@pytest.mark.parametrize("empty", [(1,), "all"], ids=["one_image_without_targets", "no_targets"])
def test_rows_path_with_empty_images(cname, B, empty):
    _check_case(cname, B, "openvocab", empty=empty, tag=str(empty))          # (PushPullLoss, like the reference, takes no image without targets)


@pytest.mark.parametrize("kind", ["pushpull", "openvocab"])
@pytest.mark.parametrize("cname,B", [("tiny", 2), ("small", 3)])
@pytest.mark.parametrize("variant", ["frozen_box_head", "floor_heads", "one_stream", "two_streams"])
def test_rows_path_in_every_combination_the_dense_section_handles(cname, B, kind, variant):
    kw = {"frozen_box_head": dict(trainable=FROZEN_BOX), "floor_heads": dict(trainable=HEADS_ONLY), "one_stream": dict(encoder_streams=1),
          "two_streams": dict(encoder_streams=2)}[variant]
    _check_case(cname, B, kind, tag=variant, **kw)


@pytest.mark.parametrize("kind", ["pushpull", "openvocab"])
def test_unmarked_gradient_takes_the_dense_path_bitwise(kind):
    cname, B = "small", 2
    s = _inputs(cname, B)
    model = _model(s, kind)
    dense = _backward(model, s, B, kind, (), "dense")
    un = _backward(model, s, B, kind, (), "auto", upstream="unmarked")
    assert un["path"] == "dense"
    assert torch.equal(dense["fg"].view(torch.int32), un["fg"].view(torch.int32))
    assert "box_rows" not in model._ws[("bwd", B)]          # the row path's workspaces were never made


def test_dense_workspaces_wait_for_a_dense_backward():
    s = _inputs("small", 2)
    model = _model(s, "pushpull")
    _backward(model, s, 2, "pushpull", (), "auto")
    bw = model._ws[("bwd", 2)]
    assert "du1" in bw and "du0" not in bw and "box_rows" in bw          # (the row path reads the dense du1; the dense du0 is never formed)
    _backward(model, s, 2, "pushpull", (), "dense")
    assert "du0" in bw


def test_broken_promise_is_loud():
    """A mark that promises fewer rows than are non-zero: NaN in dense0's gradients and in everything below d(feats), no exception, no sync."""
    cname, B = "small", 2
    s = _inputs(cname, B)
    model = _model(s, "pushpull")
    model.finish()
    model.flat_grad.zero_()
    run, pb, cl = _loss(model, s, B, "pushpull", ())
    p2, c2 = pb.detach().clone().requires_grad_(True), cl.detach().clone().requires_grad_(True)
    run(p2, c2).backward()
    assert int((p2.grad.reshape(-1, 4) != 0).any(dim=1).sum()) > 1
    torch.autograd.backward([pb, cl], [autograd.mark_box_rows(p2.grad.clone(), 1), c2.grad])
    torch.cuda.synchronize()
    assert model.last_box_backward == "rows"
    for n in ("box_head.dense0.weight", "box_head.dense0.bias", "backbone.encoder.layers.11.mlp.fc2.weight"):
        assert bool(torch.isnan(model.p(n).grad).any()), n


def test_box_backward_switch_is_validated():
    s = _inputs("tiny", 2)
    model = _model(s, "pushpull")
    model.box_backward = "sparse"
    run, pb, cl = _loss(model, s, 2, "pushpull", ())
    with pytest.raises(ValueError, match="box_backward"):
        run(pb, cl).backward()
