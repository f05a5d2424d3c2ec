"""CPU: the surface of OWLv2's objectness head that needs no device -- weights.hf_objectness_head on an Owlv2ForObjectDetection state dict's names, the
KeyError on an OWL-ViT one, from_hf_state_dict still skipping the six tensors, the two C entries' argument validation, the header's exports, the
wrappers and model methods present with the signatures the issue names."""
import inspect

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd import _lib, autograd, models, ops, postprocess, weights
from owl_vit_object_detection_amd.config import get_config, get_text_config
from tests.golden.make_golden_objectness import objectness_head
from tests.golden.make_golden_owlv2 import v2_state_dict


def test_hf_objectness_head_on_the_v2_names():
    cfg = get_config("tiny")
    D = cfg.hidden
    sd = v2_state_dict(cfg, get_text_config("tiny"))
    want = objectness_head(cfg, 5)
    for k in weights.OBJECTNESS_HEAD_KEYS:
        sd["objectness_head." + k] = torch.from_numpy(np.asarray(want[k]).reshape(sd["objectness_head." + k].shape))          # HF's [1, D] / [1] for dense2
    head = weights.hf_objectness_head(sd)
    assert tuple(head) == weights.OBJECTNESS_HEAD_KEYS == ("dense0.weight", "dense0.bias", "dense1.weight", "dense1.bias", "dense2.weight", "dense2.bias")
    assert [head[k].shape for k in head] == [(D, D), (D,), (D, D), (D,), (D,), ()]
    for k in head:
        assert head[k].dtype == np.float32 and np.array_equal(head[k], np.asarray(want[k]).reshape(head[k].shape)), k
    assert not any("objectness" in k for k in weights.from_hf_state_dict(sd))          # the vision path still does not own them


def test_an_owlvit_state_dict_has_no_objectness_head():
    sd = {k: v for k, v in v2_state_dict(get_config("tiny")).items() if not k.startswith("objectness_head.")}
    with pytest.raises(KeyError, match=r"objectness_head\.dense0\.weight.*OWL-ViT checkpoint has no objectness head"):
        weights.hf_objectness_head(sd)
    sd = v2_state_dict(get_config("tiny"))
    del sd["objectness_head.dense1.bias"]
    with pytest.raises(KeyError, match=r"objectness_head\.dense1\.bias"):
        weights.hf_objectness_head(sd)


def test_header_exports_and_argument_validation():
    protos = _lib.parse_header()
    assert [t for t, _ in protos["owl_objectness_final_fwd"][1]] == ["void*", "const void*", "const float*", "const float*", "float*", "int64_t", "int64_t"]
    assert [n for _, n in protos["owl_objectness_final_bwd"][1]] == ["stream", "dlogits", "h1_bf16", "u1_bf16", "w2", "du1_bf16", "partials", "dw2_db2", "rows", "D",
                                                                    "du1_colsum"]
    assert protos["owl_objectness_final_bwd_blocks"][1] == [("int64_t", "rows")]
    assert _lib.header_abi_version() == 8          # additive entries: the version stays
    lib = _lib.load()
    assert (lib.owl_objectness_final_bwd_blocks(1), lib.owl_objectness_final_bwd_blocks(4096), lib.owl_objectness_final_bwd_blocks(4100),
            lib.owl_objectness_final_bwd_blocks(115200)) == (1, 512, 456, 1800)
    h = torch.zeros(8)          # host memory nothing reads: the checks run before any launch
    with pytest.raises(_lib.OwlLibError, match="owl_objectness_final_fwd: null pointer"):
        _lib.call("owl_objectness_final_fwd", None, None, h, h, h, 1, 8)
    with pytest.raises(_lib.OwlLibError, match="owl_objectness_final_bwd: null pointer"):
        _lib.call("owl_objectness_final_bwd", None, h, h, h, h, h, None, h, 1, 8, None)
    for D in (0, 4, 12, 1032, 2048):
        with pytest.raises(_lib.OwlLibError, match="8 <= D <= 1024"):
            _lib.call("owl_objectness_final_fwd", None, h, h, h, h, 1, D)
        with pytest.raises(_lib.OwlLibError, match="8 <= D <= 1024"):
            _lib.call("owl_objectness_final_bwd", None, h, h, h, h, h, h, h, 1, D, None)
    with pytest.raises(_lib.OwlLibError, match="rows >= 1"):
        _lib.call("owl_objectness_final_fwd", None, h, h, h, h, 0, 8)
    with pytest.raises(_lib.OwlLibError, match="rows >= 1"):
        _lib.call("owl_objectness_final_bwd", None, h, h, h, h, h, h, h, 0, 8, None)


def test_python_surface_is_there():
    for fn in (ops.objectness_final, ops.objectness_final_bwd, postprocess.top_objects):
        assert callable(fn)
    assert issubclass(autograd.OwlViTObjectnessFunction, torch.autograd.Function)
    M = models.OwlViT
    for name in ("detect", "detect_text", "forward_queries", "forward_text"):
        p = inspect.signature(getattr(M, name)).parameters["objectness"]
        assert p.default is False, name
    assert inspect.signature(M.set_objectness_head).parameters["trainable"].default is False
    lm = inspect.signature(models.load_model).parameters
    assert lm["objectness_head"].default is None and lm["objectness_head_trainable"].default is False
    for name in ("objectness_head_parameters", "objectness_head_state"):
        assert callable(getattr(M, name))


def test_top_objects_validates_its_arguments():
    b, o = torch.zeros(2, 9, 4), torch.zeros(2, 9)
    with pytest.raises(ValueError, match="pred_boxes \\[B, P, 4\\] and objectness_logits \\[B, P\\]"):
        postprocess.top_objects(b, torch.zeros(2, 8), 3)
    for k in (0, 10):
        with pytest.raises(ValueError, match="1 <= k <= 9"):
            postprocess.top_objects(b, o, k)
