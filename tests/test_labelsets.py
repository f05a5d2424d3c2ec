"""Label sets beyond 10 classes, the part that needs no GPU: the oracle against the reference fixture f11_tiny_c80 (tiny config, 80 classes; made by
tests/golden/make_golden_labelsets.py), the C ABI of the wide class head, and the host-side sizing."""
import os

import numpy as np
import pytest
import torch

from oracle import owl_oracle as O
from owl_vit_object_detection_amd import _lib, ops, synth, weights
from owl_vit_object_detection_amd.config import get_config

LOSS_KEYS = ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")
WIDE_ENTRIES = ("owl_query_normalize_wide", "owl_class_sims_wide_fwd", "owl_class_sims_wide_bwd", "owl_query_normalize_wide_bwd")


def test_oracle_matches_f11_tiny_c80(golden_dir):
    """fp32 oracle vs the reference's own outputs at 80 classes, at tests/test_oracle_golden.py's tolerances (outputs 2e-5)."""
    g = np.load(os.path.join(golden_dir, "f11_tiny_c80.npz"))
    assert all(isinstance(g[k], np.ndarray) for k in g.files) and os.path.getsize(os.path.join(golden_dir, "f11_tiny_c80.npz")) < 1 << 20
    cfg = get_config("tiny", n_classes=int(g["n_classes"]))
    assert cfg.n_classes == 80 and len({int(l) // 10 for l in g["tgt_labels"]}) >= 3
    seed = int(g["seed"])
    w = {k: torch.from_numpy(v) for k, v in weights.make_weights(cfg, seed).items()}
    img = torch.from_numpy(synth.make_images(cfg, 1, seed))
    labels, boxes = [g["tgt_labels"]], [g["tgt_boxes"]]
    scales = torch.from_numpy(synth.class_scales(cfg, labels))
    assert np.array_equal(scales.numpy(), g["scales"])
    lab = [torch.from_numpy(l) for l in labels]
    tb = [torch.from_numpy(b) for b in boxes]
    (pb, ps), losses, grads = O.train_step(cfg, w, img, lab, tb, scales)
    np.testing.assert_allclose(pb.numpy(), g["pred_boxes"], atol=2e-5)
    np.testing.assert_allclose(ps.numpy(), g["pred_sims"], atol=2e-5)
    details = []
    O.push_pull_loss(ps, lab, pb, tb, cfg.n_classes, scales, details)
    assert np.array_equal(details[0]["pred_idx"].numpy(), g["pred_idx"]) and np.array_equal(details[0]["tgt_idx"].numpy(), g["tgt_idx"])
    assert np.array_equal(details[0]["target_classes_matched"].numpy(), g["target_classes_matched"])
    assert np.array_equal(details[0]["target_classes"].numpy(), g["target_classes"])
    for k in LOSS_KEYS:
        assert float(losses[k]) == pytest.approx(float(g[k]), rel=2e-4, abs=1e-6), k
    names = [k[5:] for k in g.files if k.startswith("grad/")]
    assert set(names) == set(grads.keys()) and len(names) == 29
    # per tensor rtol 1e-3 + 1e-4 of its largest element; a tensor whose true gradient is zero (k_proj.bias: softmax ignores a key bias) holds only the
    # rounding noise of sums of O(gmax) terms, which differs from one CPU to the next: it is judged against one f32 ulp (1.2e-7) of the largest gradient element
    gmax = max(float(np.abs(g["grad/" + n]).max()) for n in names)
    for n in names:
        ref = g["grad/" + n]
        np.testing.assert_allclose(grads[n].numpy(), ref, rtol=1e-3, atol=max(1e-4 * float(np.abs(ref).max()), 1.2e-7 * gmax), err_msg=n)
    for k in ("gap", "coord", "inter", "iou", "simpos"):          # the margins the generator checked before writing
        assert float(g["margin/" + k]) > 0


def test_wide_entries_in_header_map_and_binding():
    protos = _lib.parse_header()
    assert _lib.header_abi_version() == 8
    for n in WIDE_ENTRIES:
        assert n in protos and protos[n][0] == "int", n
    assert [a for _, a in protos["owl_class_sims_wide_bwd"][1]][-4:] == ["rows", "Dt", "C", "Qp"]
    lib = _lib.load()
    for n in WIDE_ENTRIES:
        assert hasattr(lib, n), n
    # the narrow entries keep their limit and message; the wide ones name theirs (argument validation runs before any GPU call)
    with pytest.raises(_lib.OwlLibError, match="1 <= queries <= 32"):
        _lib.call("owl_query_normalize", None, 1, 1, None, 33, 64)
    with pytest.raises(_lib.OwlLibError, match="3\\*C <= 32"):
        _lib.call("owl_class_sims_fwd", None, 1, 1, 1, None, None, 8, 64, 11)
    with pytest.raises(_lib.OwlLibError, match="C <= 384"):
        _lib.call("owl_query_normalize_wide", None, 1, 1, None, 3 * 385, 64)
    with pytest.raises(_lib.OwlLibError, match="C <= 384"):
        _lib.call("owl_class_sims_wide_fwd", None, 1, 1, 1, None, None, 8, 64, 385)
    with pytest.raises(_lib.OwlLibError, match="Qp"):
        _lib.call("owl_class_sims_wide_bwd", None, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 64, 80, 288)


def test_wide_layout_sizes():
    assert [ops.wide_blocks(c) for c in (1, 10, 11, 20, 80, 91, 384)] == [1, 1, 2, 2, 8, 10, 39]
    assert [ops.wide_qp(c) for c in (11, 80, 81, 91, 384)] == [256, 256, 512, 512, 1280]
    assert ops.WIDE_MAX_CLASSES == 384


def test_slab_scratch_covers_the_prompt_gradient_product():
    """The split-K slab must hold the wide head's [Qp, Dt] prompt-gradient product on either route of autograd.weight_grad; 10 classes size it as before."""
    from owl_vit_object_detection_amd import autograd as A
    for cname in ("owlvit-base-patch16", "owlvit-large-patch14", "tiny", "small"):
        cfg = get_config(cname)
        D, I, Dt = cfg.hidden, cfg.mlp, cfg.text_dim
        before = max(A._split_k(a, b, 1 << 30) * a * b for a, b in [(3 * D, D), (D, D), (I, D), (D, I), (Dt, D), (32, Dt)])
        assert A._dw_sizes(cfg).slab == A._dw_sizes(cfg, 32).slab == before
        for C in (11, 80, 384):
            Qp = ops.wide_qp(C)
            need_nt = A._split_k(Qp, Dt, 1 << 30) * Qp * Dt
            need_tn = (256 // ((Qp // 256) * (Dt // 256))) * Qp * Dt if Dt % 256 == 0 else 0
            assert A._dw_sizes(cfg, Qp).slab >= max(need_nt, need_tn) and A._dw_plan(Qp, Dt).slab_elems >= max(need_nt, need_tn)


def test_385_classes_are_refused_at_construction():
    from owl_vit_object_detection_amd.models import OwlViT
    with pytest.raises(ValueError, match="384"):
        OwlViT(get_config("tiny", n_classes=385), {}, "cpu")
    with pytest.raises(ValueError, match="384"):
        OwlViT(get_config("tiny", n_classes=0), {}, "cpu")
