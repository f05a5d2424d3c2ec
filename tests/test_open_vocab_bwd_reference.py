"""CPU: the checker of the open-vocabulary class head's backward (tests/open_vocab_bwd_reference.py).

* the float64 closed form equals torch autograd of HF's own OwlViTClassPredictionHead (live transformers, module in .double()) to 1e-12 relative to each
  tensor's largest element: per-image and shared banks, masks, padded all-zero queries, and an all-zero e row (1 / eps-scaled, compared on its own);
* the f32 simulation of the kernels passes the derived bounds on every shape and variant of the GPU test, and every planted error is caught by them;
* the C ABI's argument checks and workspace size (they run before any HIP call)."""
import os

import pytest
import torch

from owl_vit_object_detection_amd import _lib
from tests import open_vocab_bwd_reference as R
from tests.test_open_vocab_reference import _hf_head


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("B,P,Q,Dt,D,shared", [(1, 4, 1, 64, 128, False), (3, 36, 33, 192, 128, False), (2, 7, 5, 64, 32, False), (3, 36, 33, 192, 128, True),
                                               (2, 7, 5, 64, 32, True)])
def test_closed_form_equals_hf_autograd_in_float64(B, P, Q, Dt, D, shared):
    head = _hf_head(D, Dt, seed=B + Q)
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        head.dense0.bias.zero_()          # (so that a zero feature row gives an all-zero e row)
    f = torch.randn(B, P, D, generator=gen, dtype=torch.float64)
    zrow = min(1, P - 1)
    f[0, zrow] = 0.0
    q = torch.randn(Q if shared else B * Q, Dt, generator=gen, dtype=torch.float64).view(*(() if shared else (B,)), Q, Dt)
    q = q * torch.logspace(-2, 1, Q, dtype=torch.float64)[:, None]
    if Q >= 3:
        q[..., Q // 2, :] = 0.0          # HF's padded query: an all-zero row
    mask = torch.rand(B, Q, generator=gen) > 0.3
    mask[:, 0] = True
    if Q >= 3:
        mask[0, Q // 2] = False          # masked on image 0, live (and still all-zero) elsewhere
    g = (0.1 * torch.randn(B, P, Q, generator=gen)).float()          # (HF casts the masked logits to f32: an f32 cotangent passes through exactly)
    f.requires_grad_(True)
    q.requires_grad_(True)
    kept = {}
    hook = head.dense0.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.__setitem__("e", o)) and None)
    logits, _ = head(f, q[None].expand(B, -1, -1) if shared else q, mask)
    hook.remove()
    (logits * g.to(logits.dtype)).sum().backward()
    e = kept["e"]
    with torch.no_grad():
        shift = head.logit_shift(f).reshape(-1)
        scale = torch.nn.functional.elu(head.logit_scale(f)).reshape(-1) + 1.0
        assert scale.min() < 1.0 < scale.max()
        r = R.exact_bwd(g, e.detach().reshape(B * P, Dt), q.detach(), shift, scale, head.logit_shift.weight, head.logit_scale.weight, B, P,
                        mask.to(torch.uint8), eps=1e-6)
        assert float(e.detach()[0, zrow].abs().max()) == 0.0
        de_hf = e.grad.reshape(B * P, Dt)
        df_hf = f.grad.reshape(B * P, D)
        df = r["dfeats"] + r["de"] @ head.dense0.weight          # the head's own d(feats) = the shift / scale term + dense0's dX
        rows = torch.ones(B * P, dtype=torch.bool)
        rows[zrow] = False
        for name, got, ref in (("de", r["de"], de_hf), ("dfeats", df, df_hf)):
            assert float((got[rows] - ref[rows]).abs().max()) <= 1e-12 * float(ref[rows].abs().max()), name
            assert float(ref[zrow].abs().max()) > 1e3 * float(ref[rows].abs().max())          # the all-zero row is 1 / eps-scaled ...
            assert float((got[zrow] - ref[zrow]).abs().max()) <= 1e-12 * float(ref[zrow].abs().max()), name + " (all-zero e row)"          # ... and compared on its own
        assert not bool(torch.isnan(r["de"]).any())
        assert float((r["dq"] - q.grad).abs().max()) <= 1e-12 * float(q.grad.abs().max())
        if Q >= 3:
            assert bool((r["dq"][0, Q // 2] == 0).all()) if not shared else True          # padded and masked: exactly 0


VARIANTS = {"plain": {}, "shared": dict(shared=True, shared_mask=True), "zero_row": dict(zero_row=True), "underflow": dict(underflow=True),
            "poison": dict(poison=True)}


def _run(case, hooks=(), seed=3, **kw):
    B, P = case[0], case[1]
    i = R.make_inputs(*case, seed=seed, **kw)
    r = R.exact_of(i, B, P)
    out = R.emulate_bwd(i["g"], i["e"], i["queries"], i["rowstats"][:, 0], i["rowstats"][:, 1], i["w_shift"], i["w_scale"], B, P, i["mask"], hooks=hooks)
    return i, r, out


SIM = [(c, "plain") for c in R.GPU_CASES] + [(c, v) for c in (R.GPU_CASES[1], R.GPU_CASES[4]) for v in VARIANTS if v != "plain"]


@pytest.mark.parametrize("case,variant", SIM)
def test_simulation_passes_the_bound(case, variant):
    i, r, (de, dfeats, dq) = _run(case, **VARIANTS[variant])
    for t in (de, dfeats, dq):
        assert bool(torch.isfinite(t).all())
    worst = R.check_bwd(f"simulation {case} {variant}", de, dfeats, dq, r)
    b = R.bounds(r)
    # the bounds are tight enough to mean something: f32 round-off of the outputs' own size for dfeats and dq, bf16 round-off for de
    rel = {k: float((b[k] / r[k].abs().max().clamp_min(1e-30)).max()) for k in ("dfeats", "dq")}
    print(f"simulation {case} {variant}: err / tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; largest tol / max |ref| dfeats {rel['dfeats']:.1e} dq {rel['dq']:.1e}")
    # (4096 queries: a worst-case chain of 4099 roundings over sums that cancel to a fraction of their terms; still 1e-2 of the largest element)
    lim = 1e-3 if case[2] <= 70 else 5e-2
    assert rel["dfeats"] < lim and rel["dq"] < lim
    assert max(worst.values()) <= 1.0


PLANTS = {"unit_jacobian": {}, "elu_one": {}, "mask_multiply": dict(poison=True), "no_shift": {}, "logit_over_scale": dict(underflow=True), "bank0": {},
          "dq_image0": dict(shared=True, shared_mask=True), "row_neighbour": {}, "bf16_acc": {}}


@pytest.mark.parametrize("hook", R.HOOKS)
def test_planted_errors_are_caught(hook):
    caught = []
    for case in (R.GPU_CASES[1], R.GPU_CASES[4]):
        i, r, (de, dfeats, dq) = _run(case, hooks=(hook,), **PLANTS[hook])
        fails = []
        R.check_bwd(f"{hook} {case}", de, dfeats, dq, r, fails)
        if fails:
            caught.append((case, [m.split(":")[0] for m in fails]))
    print(hook, caught)
    assert caught, f"planted error `{hook}` passes the bounds on every case"


def test_forward_queries_validates_on_the_host():
    """Where no kernel is reached: the missing head, detect's shape checks, the id layouts forward_text shares with detect_text."""
    import types
    from owl_vit_object_detection_amd import models
    from owl_vit_object_detection_amd.config import get_config
    img = torch.zeros(2, 3, 96, 96)
    with pytest.raises(RuntimeError, match="forward_queries: no logit head.*set_logit_head"):
        models.OwlViT.forward_queries(types.SimpleNamespace(logit_head=None), img, torch.zeros(2, 5, 64))
    stub = types.SimpleNamespace(logit_head={}, cfg=get_config("tiny"))
    with pytest.raises(ValueError, match=r"query_embeds must be \[2, Q, 64\] or \[Q, 64\]"):
        models.OwlViT.forward_queries(stub, img, torch.zeros(3, 5, 64))
    with pytest.raises(ValueError, match=r"query_mask must be \[2, 5\] or \[5\]"):
        models.OwlViT.forward_queries(stub, img, torch.zeros(2, 5, 64), torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"forward_text: input_ids must be \[2, Q, S\]"):
        models.OwlViT.forward_text(stub, img, torch.zeros(3, 5, 16, dtype=torch.int64), None)
    with pytest.raises(ValueError, match=r"forward_text: input_ids \[5, S\] is not \[2 Q, S\]"):
        models.OwlViT.forward_text(stub, img, torch.zeros(5, 16, dtype=torch.int64), None, shared=False)
    # one parser for both entries: the layouts and the mask rule of detect_text
    tower = types.SimpleNamespace(encode=lambda ids: torch.ones(ids.shape[0], 64))
    ids = torch.zeros(2, 3, 16, dtype=torch.int64); ids[0, :, 0] = 7; ids[1, 0, 0] = 7
    emb, mask = models.text_queries("detect_text", 2, ids, tower)
    assert emb.shape == (2, 3, 64) and mask.tolist() == [[True, True, True], [True, False, False]]
    emb2, mask2 = models.text_queries("forward_text", 2, ids.reshape(6, 16), tower)
    assert torch.equal(emb, emb2) and torch.equal(mask, mask2)
    emb3, mask3 = models.text_queries("forward_text", 2, ids[0], tower, shared=True)
    assert emb3.shape == (3, 64) and mask3.tolist() == [True, True, True]


def test_split_is_a_function_of_p_and_q_alone():
    assert R.split(4, 1) == (1, 32) and R.split(70, 70) == (3, 32) and R.split(2304, 30) == (36, 64) and R.split(2304, 1203) == (1, 2304) and R.split(4, 4096) == (1, 32)


def test_abi_argument_checks(built):
    nbytes = torch.zeros(1, dtype=torch.int64)
    _lib.call("owl_class_logits_bwd_workspace_bytes", 3, 36, 33, 3, 192, 1, nbytes)
    S, chunk = R.split(36, 33)
    Qp = 64
    assert int(nbytes) == 4 * (3 * Qp * 192 + 2 * 3 * Qp + 108 + 3 * S * Qp * 192)
    _lib.call("owl_class_logits_bwd_workspace_bytes", 3, 36, 33, 1, 192, 0, nbytes)
    assert int(nbytes) == 4 * (Qp * 192 + 2 * Qp + 108)
    for args, word in (((3, 36, 0, 3, 192, 1), "Q"), ((3, 36, 4097, 3, 192, 1), "Q"), ((3, 36, 33, 3, 96, 1), "Dt"), ((3, 36, 33, 3, 2048, 1), "Dt"),
                       ((3, 8193, 33, 3, 192, 1), "P"), ((3, 36, 33, 2, 192, 1), "nbanks")):
        with pytest.raises(_lib.OwlLibError, match=word):
            _lib.call("owl_class_logits_bwd_workspace_bytes", *args, nbytes)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_class_logits_bwd", None, None, None, None, None, None, None, None, None, 0, None, None, None, 1, 4, 1, 1, 1, 64, 128)
