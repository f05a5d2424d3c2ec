"""The weight-gradient planner (autograd._dw_plan) and the scratch sized from it (autograd._dw_sizes), against the library's own host-side workspace
queries: whatever route and split count the planner picks, the slab of the lane that runs the product holds what the kernels write, and the scratch the NT
route needs exists.  No device: the sizing is a pure function of the config, the routed width and the trainable-embeddings flag."""
import itertools

import pytest
import torch

from owl_vit_object_detection_amd import _lib, ops
from owl_vit_object_detection_amd import autograd as A
from owl_vit_object_detection_amd.config import CONFIGS, get_config

CASES = [get_config(n) for n in CONFIGS] + [get_config("owlvit-base-patch16", text_dim=256), get_config("small", text_dim=256)]
SWITCHES = [(True, 256), (False, 256), (True, 64), (True, 1024)]          # (TN_SMALL_N, DW_ITEMS)


def _written(plan, rows, n_out):
    """f32 elements the library says the planned call writes."""
    b = torch.zeros(1, dtype=torch.int64)
    if plan.tn:
        _lib.call("owl_gemm_tn_slab_workspace_bytes", rows, n_out, plan.n_in_pad, plan.splits, b)
    else:
        _lib.call("owl_gemm_slab_workspace_bytes", n_out, plan.n_in_pad, ops.pad_rows(rows), plan.splits, b)
    return int(b.item()) // 4


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: f"{c.name}-Dt{c.text_dim}")
def test_scratch_covers_every_planned_product(cfg, monkeypatch):
    D, I, Dt = cfg.hidden, cfg.mlp, cfg.text_dim
    for C, emb, (small_n, items) in itertools.product((cfg.n_classes, 11, 80, 384), (False, True), SWITCHES):
        monkeypatch.setattr(A, "TN_SMALL_N", small_n)
        monkeypatch.setattr(A, "DW_ITEMS", items)
        c = cfg.replace(n_classes=C)
        Qg = ops.wide_qp(C) if C > 10 else 32
        sz = A._dw_sizes(c, Qg, emb)
        # (n_out, n_in, bias gradients it is launched with, slabs of the lanes it can run on, transposed-operand pair rows (dy^T, x^T) at token / head rows)
        tok, head = (sz.tok_rows, sz.tok_rows), (sz.tAh_rows, sz.tBh_rows)
        products = [(3 * D, D, (True,), (sz.slab,), (tok,)), (I, D, (True,), (sz.slab,), (tok,)), (D, I, (False,), (sz.slab,), (tok,)),
                    (D, D, (False, True), (sz.slab,), (tok, head)),                       # out_proj at token rows, the box head's two at head rows
                    (Dt, D, (True,), (sz.slab, sz.slab2), (head,)), (Qg, Dt, (False,), (sz.slab, sz.slab2), (head,))]
        if emb:
            products.append((D, c.patch_k, (False,), (sz.slab,), (head,)))
        for (n_out, n_in, biases, slabs, pairs), bias, B in itertools.product(products, (False, True), (1, 3, 64)):
            if bias not in biases:
                continue
            for rows in (B * c.patches, B * c.tokens_padded):
                plan = A._dw_plan(n_out, n_in, bias=bias, tn_all=sz.tn_all, rows=rows)
                need = _written(plan, rows, n_out)
                assert need <= plan.slab_elems and all(need <= s for s in slabs), (C, emb, small_n, items, n_out, n_in, rows, plan, need, sz)
                if not plan.tn:
                    assert plan.n_in_pad % 8 == 0 and 0 <= plan.n_in_pad - n_in < 8
                    assert all(a >= n_out and b >= n_in for a, b in pairs), (C, emb, small_n, n_out, n_in, plan, sz)


def test_both_routes_and_the_padded_product_are_reached():
    """The cases above are not all on one route: B/16 is all TN (the 32-row prompt product included), tiny all NT, and L/14's patch product runs 8-padded."""
    assert all(A._dw_plan(a, b).tn for a, b in [(2304, 768), (768, 768), (3072, 768), (768, 3072), (512, 768)])
    assert A._dw_plan(32, 512, tn_all=True).tn and not A._dw_plan(32, 512, tn_all=True, bias=True).tn and not A._dw_plan(32, 512).tn
    assert not any(A._dw_plan(a, b).tn for a, b in [(384, 128), (128, 128), (256, 128), (128, 256), (64, 128), (32, 64)])
    p = A._dw_plan(1024, 588)
    assert not p.tn and p.n_in_pad == 592 and p.slab_elems == p.splits * 1024 * 592


def test_class_head_lane_holds_the_tn_route_at_text_dim_256():
    """text_dim = 256 with a hidden size that is a multiple of 256: the class head's weight gradient is on the TN route with 256 // 3 = 85 splits of
    256 x 768 floats; the NT formula for that shape (42 splits) is too small."""
    sz = A._dw_sizes(get_config("owlvit-base-patch16", text_dim=256))
    plan = A._dw_plan(256, 768, bias=True, tn_all=sz.tn_all)
    assert plan.tn and plan.splits == 85 and 42 * 256 * 768 < 85 * 256 * 768 == 16711680 <= min(sz.slab, sz.slab2)


def test_shipped_configs_keep_their_slab_sizes():
    """Split-K slab elements (main, class-head lane) of the four configs the benchmarks and parity tests run, 10 classes or fewer, embeddings frozen."""
    want = {"owlvit-base-patch16": (16515072, 16515072), "owlvit-large-patch14": (16777216, 16515072), "tiny": (8388608, 4194304), "small": (16777216, 8388608)}
    for name, slabs in want.items():
        sz = A._dw_sizes(get_config(name))
        assert (sz.slab, sz.slab2) == slabs, (name, sz)
