"""CPU side of the selectable trainable set (`trainable=`): the freeze rule's semantics, unit validation, the bucket layout and the stated work."""
import numpy as np
import pytest

from owl_vit_object_detection_amd import models, weights
from owl_vit_object_detection_amd.config import get_config

HEADS = ("box", "post_layernorm", "class_predictor", "queries")
EVERYTHING = ("backbone", "post_post_layernorm", "class_predictor", "box_head", "queries")
SETS = [None, weights.FREEZE_KEEP, ("layers.10.", "layers.11.") + HEADS, ("layers.13.",) + HEADS, ("layers.11.", "layers.13.") + HEADS, ("queries",),
        ("queries", "class_predictor", "box"), ("layers.1",) + HEADS, ("pre_layernorm", "layers.0."), EVERYTHING]


def _reference_rule(names, keep):
    """Literal transcription of the reference's loop (src/models.py:173-184): freeze everything, then unfreeze by substring."""
    out = {}
    for name in names:
        requires_grad = False
        for s in keep:
            if s in name:
                requires_grad = True
        out[name] = requires_grad
    return out


@pytest.mark.parametrize("keep", [weights.FREEZE_KEEP, ("layers.1",), ("layers.23", "queries"), ("box", "class_predictor"), ("backbone",), ("weight",), ()])
def test_is_trainable_is_the_reference_loop(keep):
    for cname in ("tiny-l14", "owlvit-large-patch14"):
        names = list(weights.param_shapes(get_config(cname)))
        ref = _reference_rule(names, keep)
        assert {n: weights.is_trainable(n, keep) for n in names} == ref
    assert all(weights.is_trainable(n) == weights.is_trainable(n, weights.FREEZE_KEEP) for n in names)


def test_layers_1_selects_layers_1_and_10_to_19_as_in_the_reference():
    cfg = get_config("owlvit-large-patch14")
    units, layers = weights.trainable_units(cfg, ("layers.1",))
    assert layers == (1, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19) and units == set(layers)
    assert weights.trainable_units(get_config("tiny"), ("layers.1",) + HEADS)[1] == (1, 10, 11)
    assert weights.trainable_units(cfg, ("layers.1.",))[1] == (1,)


def test_partial_units_and_empty_sets_raise():
    cfg = get_config("tiny")
    with pytest.raises(ValueError, match=r"part of the unit `box_head`.*box_head\.dense1\.weight"):
        weights.trainable_units(cfg, ("box_head.dense0", "box_head.dense2"))
    with pytest.raises(ValueError, match=r"part of the unit `backbone\.encoder\.layers\.3`.*layers\.3\.mlp\.fc1\.weight"):
        weights.trainable_units(cfg, ("layers.3.self_attn", "layers.3.layer_norm"))
    with pytest.raises(ValueError, match=r"part of the unit `backbone\.embeddings`.*class_embedding"):
        weights.trainable_units(cfg, ("position_embedding", "patch_embedding"))
    with pytest.raises(ValueError, match=r"part of the unit"):
        weights.trainable_units(cfg, ("weight",))
    for empty in ((), ("layers.12",), ("no_such_tensor",)):
        with pytest.raises(ValueError, match="selects no parameter"):
            weights.trainable_units(cfg, empty)
    with pytest.raises(ValueError, match="iterable of substrings"):
        weights.trainable_units(cfg, "queries")


def test_backward_floor_names_the_lowest_point_of_the_chain():
    cfg = get_config("tiny-l14")
    floor = lambda keep: weights.backward_floor(weights.trainable_units(cfg, keep)[0])
    assert floor(None) == 11 and floor(("layers.13.",) + HEADS) == 13 and floor(("layers.11.", "layers.13.")) == 11
    assert floor(("queries",)) == "heads" and floor(("box", "class_predictor")) == "heads"
    assert floor(("post_post_layernorm",)) == "post_post_layernorm" and floor(("post_layernorm",)) == "post_layernorm"
    assert floor(("pre_layernorm", "queries")) == "pre_layernorm" and floor(("embeddings",)) == "embeddings" and floor(EVERYTHING) == "embeddings"


# the bucket layout of the reference set: checkpoints and FusedAdamW states are written against these offsets
_REFERENCE_ORDER = [
    "queries",
    "backbone.encoder.layers.11.self_attn.q_proj.weight", "backbone.encoder.layers.11.self_attn.k_proj.weight", "backbone.encoder.layers.11.self_attn.v_proj.weight",
    "backbone.encoder.layers.11.self_attn.q_proj.bias", "backbone.encoder.layers.11.self_attn.k_proj.bias", "backbone.encoder.layers.11.self_attn.v_proj.bias",
    "backbone.encoder.layers.11.self_attn.out_proj.weight", "backbone.encoder.layers.11.self_attn.out_proj.bias",
    "backbone.encoder.layers.11.layer_norm1.weight", "backbone.encoder.layers.11.layer_norm1.bias",
    "backbone.encoder.layers.11.mlp.fc1.weight", "backbone.encoder.layers.11.mlp.fc1.bias", "backbone.encoder.layers.11.mlp.fc2.weight", "backbone.encoder.layers.11.mlp.fc2.bias",
    "backbone.encoder.layers.11.layer_norm2.weight", "backbone.encoder.layers.11.layer_norm2.bias",
    "backbone.post_layernorm.weight", "backbone.post_layernorm.bias", "post_post_layernorm.weight", "post_post_layernorm.bias",
    "class_predictor.dense0.weight", "class_predictor.dense0.bias",
    "box_head.dense0.weight", "box_head.dense0.bias", "box_head.dense1.weight", "box_head.dense1.bias", "box_head.dense2.weight", "box_head.dense2.bias",
]


@pytest.mark.parametrize("cname", ["tiny", "tiny-l14", "owlvit-base-patch16", "owlvit-large-patch14"])
def test_flat_order_of_the_reference_set_is_pinned(cname):
    cfg = get_config(cname)
    assert models._flat_order(cfg) == _REFERENCE_ORDER == models._flat_order(cfg, weights.FREEZE_KEEP) and len(_REFERENCE_ORDER) == 29


def _offsets(cfg, keep):
    shapes = weights.param_shapes(cfg)
    offs, off = {}, 0
    for n in models._flat_order(cfg, keep):
        offs[n] = (off, int(np.prod(shapes[n])))
        off += (offs[n][1] + 7) // 8 * 8          # models.OwlViT.__init__'s rule
    return offs, off


@pytest.mark.parametrize("keep", SETS)
def test_flat_order_covers_the_set_with_aligned_disjoint_offsets(keep):
    cfg = get_config("tiny-l14")
    order = models._flat_order(cfg, keep)
    want = {n for n in weights.param_shapes(cfg) if weights.is_trainable(n, weights.FREEZE_KEEP if keep is None else keep)}
    assert set(order) == want and len(order) == len(set(order))
    if "queries" in want:
        assert order[0] == "queries"
    offs, total = _offsets(cfg, keep)
    end = 0
    for n in order:
        o, numel = offs[n]
        assert o % 8 == 0 and o >= end, n          # 8-aligned, after everything before it
        end = o + numel
    assert end <= total
    # q, k, v of a trainable layer are adjacent (the fused [3D, D] views), in the per-layer order of the reference set
    D = cfg.hidden
    for n in order:
        if n.endswith("self_attn.q_proj.weight"):
            pre = n[:-len("q_proj.weight")]
            assert offs[pre + "k_proj.weight"][0] == offs[n][0] + D * D and offs[pre + "v_proj.weight"][0] == offs[n][0] + 2 * D * D
            assert offs[pre + "k_proj.bias"][0] == offs[pre + "q_proj.bias"][0] + D and offs[pre + "v_proj.bias"][0] == offs[pre + "q_proj.bias"][0] + 2 * D
            i = order.index(n)
            assert [m[len(pre) - len("self_attn."):] for m in order[i:i + 16]] == [m.split("layers.11.")[1] for m in _REFERENCE_ORDER[1:17]]
    if "box_head.dense2.weight" in want:
        assert offs["box_head.dense2.bias"][0] == offs["box_head.dense2.weight"][0] + offs["box_head.dense2.weight"][1]


# values of the parent commit (config.OwlConfig.flops_backward() before it took arguments)
_FLOPS_BACKWARD = {"owlvit-base-patch32": 22047627264.0, "owlvit-base-patch16": 112566736896.0, "owlvit-large-patch14": 2691579256832.0}


@pytest.mark.parametrize("cname", sorted(_FLOPS_BACKWARD))
def test_default_flops_are_unchanged(cname):
    cfg = get_config(cname)
    assert cfg.flops_backward() == _FLOPS_BACKWARD[cname]
    assert cfg.flops_train_step() == cfg.flops_forward() + _FLOPS_BACKWARD[cname]
    assert cfg.flops_backward(trainable_layers=(11,), floor=11) == _FLOPS_BACKWARD[cname]          # the reference set, stated
    assert cfg.trainable_layer() == 11


def test_flops_of_other_sets():
    cfg = get_config("owlvit-large-patch14")
    T, D, I = cfg.tokens, cfg.hidden, cfg.mlp
    dx_only_layer = (8.0 * T * D * D + 4.0 * T * D * I) + 2.0 * (4.0 * T * T * D)
    assert cfg.flops_backward() - cfg.flops_backward(trainable_layers=(23,), floor=23) == 12 * dx_only_layer
    assert cfg.flops_backward(trainable_layers=(), floor="heads") == 2.0 * cfg.flops_heads() == cfg.flops_backward(floor="post_layernorm")
    assert cfg.flops_backward(trainable_layers=(22, 23), floor=22) == 4.0 * cfg.flops_layer() + 2.0 * cfg.flops_heads()
    full = cfg.flops_backward(trainable_layers=tuple(range(24)), floor="embeddings")
    assert full == 48.0 * cfg.flops_layer() + 2.0 * cfg.flops_heads() + 2.0 * cfg.patches * cfg.patch_k * cfg.hidden
    assert cfg.flops_train_step(trainable_layers=(23,), floor=23) == cfg.flops_forward() + cfg.flops_backward(trainable_layers=(23,), floor=23)
