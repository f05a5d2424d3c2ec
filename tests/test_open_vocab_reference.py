"""CPU: the checker of the open-vocabulary class head (tests/open_vocab_reference.py) and the host side of zero-shot inference.

* the float64 restatement equals HF's own OwlViTClassPredictionHead (live transformers, module in .double()) to 1e-12 and fixture F15 at f32 round-off;
* the f32 simulation of the kernel passes the derived bound on every shape of the GPU test, and every planted error is caught by it;
* weights.hf_logit_head against a live HF state dict and a missing key; detect's argument validation, where no kernel is reached; the C ABI's
  argument checks (they run before any HIP call)."""
import os
import types

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd import _lib, models, ops, weights
from owl_vit_object_detection_amd.config import get_config
from tests import open_vocab_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f15_open_vocab.npz")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _hf_head(D, Dt, seed):
    from transformers import OwlViTConfig
    from transformers.models.owlvit.modeling_owlvit import OwlViTClassPredictionHead
    torch.manual_seed(seed)
    cfg = OwlViTConfig(text_config=dict(hidden_size=Dt, intermediate_size=2 * Dt, num_hidden_layers=1, num_attention_heads=1, vocab_size=97, max_position_embeddings=16),
                       vision_config=dict(hidden_size=D, intermediate_size=2 * D, num_hidden_layers=1, num_attention_heads=2, image_size=32, patch_size=16), projection_dim=Dt)
    head = OwlViTClassPredictionHead(cfg).double()
    with torch.no_grad():          # ~0 at init: give shift and scale something to do, both ELU branches
        head.logit_shift.weight.normal_(0, 0.3 / D ** 0.5); head.logit_shift.bias.fill_(0.05)
        head.logit_scale.weight.normal_(0, 1.0 / D ** 0.5); head.logit_scale.bias.fill_(0.1)
    return head


@pytest.mark.parametrize("B,P,Q,Dt,D", [(1, 4, 1, 64, 128), (3, 36, 33, 192, 128), (2, 7, 5, 64, 32)])
def test_restatement_equals_hf_module_in_float64(B, P, Q, Dt, D):
    head = _hf_head(D, Dt, seed=B + Q)
    g = torch.Generator().manual_seed(5)
    f = torch.randn(B, P, D, generator=g, dtype=torch.float64)
    q = torch.randn(B, Q, Dt, generator=g, dtype=torch.float64) * torch.logspace(-2, 1, Q, dtype=torch.float64)[None, :, None]
    q[0, Q // 2] = 0.0          # HF's padded query: an all-zero row
    mask = torch.rand(B, Q, generator=g) > 0.3
    with torch.no_grad():
        lg, _ = head(f, q, None)          # (its second output is the NORMALISED class embedding: the restatement takes dense0's own output)
        e = head.dense0(f)
        lgm, _ = head(f, q, mask)          # (HF returns float32 on this path, finfo of the compute dtype cast down)
        r = R.exact_logits(e.reshape(B * P, Dt), q, f.reshape(B * P, D), head.logit_shift.weight, head.logit_shift.bias, head.logit_scale.weight,
                           head.logit_scale.bias, B, P, mask)
    assert (x := r["x"]).min() < 0 < x.max()
    # (eps6 is the f32 nearest 1e-6, HF's literal the double: 2.5e-15 relative to a norm, nothing at 1e-12 for norms >= 1e-2)
    assert float((r["raw"] - lg).abs().max()) < 1e-12
    assert not bool(torch.isnan(r["raw"]).any()) and torch.equal(r["raw"][0, :, Q // 2], (r["shift"] * r["scale"])[0, :, 0])
    live = mask[:, None, :].expand(B, P, Q)
    assert torch.equal(r["logits"][~live], torch.full_like(r["logits"][~live], R.FMIN)) and bool((r["scores"][~live] == 0).all())
    assert float((r["logits"][live] - lgm.double()[live]).abs().max()) < 1e-6
    assert float((r["scores"][live] - torch.sigmoid(lg)[live]).abs().max()) < 1e-12


def test_restatement_equals_fixture_f15():
    g = np.load(GOLDEN)
    B, P, Q = g["logits"].shape
    head = {k: torch.from_numpy(g["head/" + k]) for k in weights.LOGIT_HEAD_KEYS}
    # (HF's class_embeds output is normalised already: e is dense0 on the stored image_embeds, its weights rebuilt by seed)
    W = weights.make_weights(get_config("tiny"))
    fe = torch.from_numpy(g["image_embeds"]).double().reshape(B * P, -1)
    e = fe @ torch.from_numpy(W["class_predictor.dense0.weight"]).double().t() + torch.from_numpy(W["class_predictor.dense0.bias"]).double()
    assert float((e / e.norm(dim=-1, keepdim=True) - torch.from_numpy(g["class_embeds"]).double().reshape(B * P, -1)).abs().max()) < 1e-5
    r = R.exact_logits(e, torch.from_numpy(g["text_embeds"]), torch.from_numpy(g["image_embeds"]).reshape(B * P, -1),
                       head["logit_shift.weight"], head["logit_shift.bias"], head["logit_scale.weight"], head["logit_scale.bias"], B, P, torch.from_numpy(g["query_mask"]))
    ref = torch.from_numpy(g["logits"]).double()
    live = r["live"].expand(B, P, Q)
    assert torch.equal(ref[~live], torch.full_like(ref[~live], R.FMIN)) and int((~live).sum()) == 2 * P
    assert float((r["logits"][live] - ref[live]).abs().max()) < 2e-6          # HF ran in f32 on these inputs: a few f32 roundings of values below 1
    # the generator's decided patches: its float64 margins rebuilt from the stored logits agree
    top = torch.where(live, ref, torch.full_like(ref, -float("inf"))).topk(2, dim=-1).values
    assert float(((top[..., 0] - top[..., 1]) - torch.from_numpy(g["margin"])).abs().max()) < 1e-5
    assert g["decided"].mean() >= 0.95
    # case B's query is the class embedding HF's embed_image_query selected, one row
    assert g["b_query_embeds"].shape == (1, g["class_embeds"].shape[-1]) and g["b_logits"].shape == (1, P, 1) and g["b_box_index"].shape == (1,)


def _sim(c, hooks=(), **kw):
    i = R.make_inputs(*c, seed=3, **kw)
    B, P = c[0], c[1]
    args = (i["e"], i["queries"], i["feats"], i["w_shift"], i["b_shift"], i["w_scale"], i["b_scale"], B, P, i["mask"])
    r = R.exact_logits(*args)
    lg, sc = R.emulate_logits(*args, hooks=hooks)
    return r, lg, sc


@pytest.mark.parametrize("case", R.GPU_CASES)
def test_simulation_passes_the_bound(case):
    """The bf16-emulated evaluation (features held in bf16, tests/bf16_emulation.bf's rounding, everything else f32 in the kernel's order) is inside the
    bound on every shape of the GPU test, and the inputs reach what they name."""
    from tests.bf16_emulation import bf
    i = R.make_inputs(*case, seed=3)
    assert torch.equal(bf(i["feats"].float()), i["feats"].float())          # the features ARE bf16 values
    r, lg, sc = _sim(case)
    assert r["x"].min() < 0 < r["x"].max() or case[0] * case[1] < 8
    assert float(r["nq"][r["nq"] > 0].min()) < 1e-2 < 1.0 < float(r["nq"].max()) or case[2] < 3
    worst = R.check_logits(f"simulation {case}", lg, sc, r)
    assert not bool(torch.isnan(lg).any())
    b = R.bounds(r)
    # the bound is tight enough to mean something: 1e-6 .. 1e-4 (the D = 1024 dot products) on logits of size ~1
    print(f"simulation {case}: err / tol logits {worst[0]:.3f} scores {worst[1]:.3f}; largest tol {float(b['logits'][r['live'].expand_as(b['logits'])].max()):.2e}")
    assert float(b["logits"][r["live"].expand_as(b["logits"])].max()) < 2e-4
    assert max(worst) <= 1.0


PLANT_CASES = [c for c in R.GPU_CASES if c[0] == 3 and c[2] >= 32]          # per-image banks and masks, several query blocks


@pytest.mark.parametrize("hook", R.HOOKS)
def test_planted_errors_are_caught(hook):
    for case in PLANT_CASES:
        r, lg, sc = _sim(case, hooks=(hook,))
        fails = []
        R.check_logits(f"{hook} {case}", lg, sc, r, fails)
        assert fails, f"{hook} passes the bound on {case}"


def test_shared_bank_is_the_repeated_bank_in_the_reference():
    c = (3, 36, 33, 192, 128)
    i = R.make_inputs(*c, seed=4, shared=True)
    a = R.exact_logits(i["e"], i["queries"], i["feats"], i["w_shift"], i["b_shift"], i["w_scale"], i["b_scale"], 3, 36, i["mask"])
    b = R.exact_logits(i["e"], i["queries"][None].repeat(3, 1, 1), i["feats"], i["w_shift"], i["b_shift"], i["w_scale"], i["b_scale"], 3, 36, i["mask"])
    assert torch.equal(a["logits"], b["logits"])
    assert R.launch_shape(4) == (1, 1) and R.launch_shape(36) == (2, 1) and R.launch_shape(576) == (6, 3) and R.launch_shape(2304) == (8, 9)


# ---- weights.hf_logit_head ----------------------------------------------------------------------------------------------------------------
def test_hf_logit_head_against_a_live_state_dict():
    from transformers import OwlViTConfig, OwlViTForObjectDetection
    torch.manual_seed(0)
    cfg = OwlViTConfig(text_config=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1, vocab_size=64, max_position_embeddings=16),
                       vision_config=dict(hidden_size=128, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, image_size=32, patch_size=16), projection_dim=64)
    hf = OwlViTForObjectDetection(cfg)
    sd = hf.state_dict()
    head = weights.hf_logit_head(sd)
    assert list(head) == list(weights.LOGIT_HEAD_KEYS)
    assert head["logit_shift.weight"].shape == (128,) and head["logit_scale.weight"].shape == (128,)
    assert head["logit_shift.bias"].shape == () and head["logit_scale.bias"].shape == ()
    for k, v in head.items():
        assert v.dtype == np.float32 and np.array_equal(v.reshape(-1), sd["class_head." + k].numpy().reshape(-1))
    as_np = weights.hf_logit_head({k: v.numpy() for k, v in sd.items()})          # numpy values, as from_hf_state_dict takes them
    assert all(np.array_equal(as_np[k], head[k]) for k in head)
    bad = {k: v for k, v in sd.items() if k != "class_head.logit_scale.bias"}
    with pytest.raises(KeyError, match="class_head.logit_scale.bias"):
        weights.hf_logit_head(bad)
    # nothing else moved: the adapter still drops them, and they are no parameters
    assert not any("logit" in k for k in weights.from_hf_state_dict(sd))
    assert not any("logit" in k for k in weights.param_shapes(get_config("tiny")))


# ---- detect: argument validation, where no kernel is reached ------------------------------------------------------------------------------------
def test_detect_without_a_logit_head_raises_before_anything_else():
    stub = types.SimpleNamespace(logit_head=None)
    with pytest.raises(RuntimeError, match="set_logit_head"):
        models.OwlViT.detect(stub, torch.zeros(1, 3, 96, 96), torch.zeros(1, 5, 64))


def test_detect_validates_shapes_naming_the_expected_one():
    cfg = get_config("tiny")
    stub = types.SimpleNamespace(logit_head={}, cfg=cfg)
    img = torch.zeros(2, 3, 96, 96)
    det = lambda *a, **k: models.OwlViT.detect(stub, *a, **k)          # noqa: E731
    with pytest.raises(ValueError, match=r"pixel_values must be \[B, 3, 96, 96\]"):
        det(torch.zeros(2, 3, 64, 96), torch.zeros(2, 5, 64))
    with pytest.raises(ValueError, match=r"query_embeds must be \[2, Q, 64\] or \[Q, 64\]"):
        det(img, torch.zeros(3, 5, 64))
    with pytest.raises(ValueError, match=r"query_embeds must be \[2, Q, 64\] or \[Q, 64\]"):
        det(img, torch.zeros(5, 32))
    with pytest.raises(ValueError, match=r"query_embeds must be \[2, Q, 64\] or \[Q, 64\]"):
        det(img, torch.zeros(64))
    with pytest.raises(ValueError, match="float32"):
        det(img, torch.zeros(5, 64, dtype=torch.float64))
    with pytest.raises(ValueError, match="1 <= Q <= 4096"):
        det(img, torch.zeros(4097, 64))
    with pytest.raises(ValueError, match="1 <= Q <= 4096"):
        det(img, torch.zeros(2, 0, 64))
    with pytest.raises(ValueError, match=r"query_mask must be \[2, 5\] or \[5\]"):
        det(img, torch.zeros(2, 5, 64), torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"query_mask must be \[2, 5\] or \[5\]"):
        det(img, torch.zeros(5, 64), torch.ones(3, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool or integer"):
        det(img, torch.zeros(5, 64), torch.ones(5))
    assert models.check_detect_args(cfg, img, torch.zeros(5, 64), torch.ones(5, dtype=torch.int64)) == (2, 5, True)
    assert models.check_detect_args(cfg, img, torch.zeros(2, 7, 64), np.ones((2, 7), bool)) == (2, 7, False)


def test_detect_text_validates_the_id_layout():
    stub = types.SimpleNamespace()
    img = torch.zeros(2, 3, 96, 96)
    with pytest.raises(ValueError, match=r"input_ids must be \[2, Q, S\]"):
        models.OwlViT.detect_text(stub, img, torch.zeros(3, 5, 16, dtype=torch.int64), None)
    with pytest.raises(ValueError, match=r"input_ids must be \[2, Q, S\]"):
        models.OwlViT.detect_text(stub, img, torch.zeros(16, dtype=torch.int64), None)
    with pytest.raises(ValueError, match=r"is not \[2 Q, S\]"):
        models.OwlViT.detect_text(stub, img, torch.zeros(5, 16, dtype=torch.int64), None, shared=False)


def test_set_logit_head_validates_on_the_host():
    stub = types.SimpleNamespace(cfg=get_config("tiny"), device_=torch.device("cpu"), logit_head="x")
    good = {"logit_shift.weight": np.zeros(128, np.float32), "logit_shift.bias": np.float32(0.5), "logit_scale.weight": torch.ones(1, 128), "logit_scale.bias": np.zeros(1)}
    models.OwlViT.set_logit_head(stub, good)
    assert list(stub.logit_head) == list(weights.LOGIT_HEAD_KEYS) and all(t.dtype == torch.float32 and t.dim() == 1 for t in stub.logit_head.values())
    assert float(stub.logit_head["logit_shift.bias"]) == 0.5 and stub.logit_head["logit_scale.weight"].shape == (128,)
    with pytest.raises(ValueError, match=r"`logit_scale.weight` must have 128"):
        models.OwlViT.set_logit_head(stub, dict(good, **{"logit_scale.weight": np.zeros(64)}))
    with pytest.raises(KeyError, match="logit_shift.bias"):
        models.OwlViT.set_logit_head(stub, {k: v for k, v in good.items() if k != "logit_shift.bias"})
    models.OwlViT.set_logit_head(stub, None)
    assert stub.logit_head is None
    import inspect
    sig = inspect.signature(models.load_model)
    assert sig.parameters["logit_head"].default is None and sig.parameters["logit_head"].kind is inspect.Parameter.KEYWORD_ONLY


# ---- the C ABI and the wrapper ---------------------------------------------------------------------------------------------------------------
def test_abi_argument_validation_without_gpu(built):
    """Argument checks run before any HIP call: safe without a device (the pointers are host memory nothing reads)."""
    h = torch.zeros(64)
    call = lambda *a: _lib.call("owl_class_logits_fwd", None, *a)          # noqa: E731
    ok = (h, h, h, h, h, h, h, None, h, h, None)
    with pytest.raises(_lib.OwlLibError, match="owl_class_logits_fwd: null pointer"):
        call(None, h, h, h, h, h, h, None, h, h, None, 1, 36, 5, 1, 1, 64, 128)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        call(h, h, h, h, h, h, h, None, None, h, None, 1, 36, 5, 1, 1, 64, 128)          # rowstats is the caller's scratch: required
    for B, P in ((0, 36), (1, 0), (1, 8193), (1 << 20, 4096)):
        with pytest.raises(_lib.OwlLibError, match="B P < 2\\^31"):
            call(*ok, B, P, 5, 1, 1, 64, 128)
    for Q in (0, 4097):
        with pytest.raises(_lib.OwlLibError, match="1 <= Q <= 4096"):
            call(*ok, 1, 36, Q, 1, 1, 64, 128)
    for Dt, D in ((0, 128), (96, 128), (64, 0), (64, 132)):
        with pytest.raises(_lib.OwlLibError, match="Dt % 64 == 0 and D % 8 == 0"):
            call(*ok, 1, 36, 5, 1, 1, Dt, D)
    with pytest.raises(_lib.OwlLibError, match="nbanks = B or 1"):
        call(*ok, 3, 36, 5, 2, 1, 64, 128)
    with pytest.raises(_lib.OwlLibError, match="nmasks = B or 1"):
        call(h, h, h, h, h, h, h, h, h, h, None, 3, 36, 5, 1, 2, 64, 128)
    with pytest.raises(_lib.OwlLibError, match="too large for the LDS-resident query table"):
        call(*ok, 1, 36, 5, 1, 1, 2048, 128)
    assert "LDS" in _lib.last_error()


def test_wrapper_refuses_host_tensors_and_bad_shapes(built):
    with pytest.raises(ValueError, match="must be a device tensor"):
        ops.class_logits(torch.zeros(36, 64), torch.zeros(5, 64), torch.zeros(36, 128, dtype=torch.bfloat16), torch.zeros(128), torch.zeros(1), torch.zeros(128),
                         torch.zeros(1), 1, 36)
    assert ops.class_logits.__doc__ and ops.CLASS_LOGITS_MAX_QUERIES == 4096
