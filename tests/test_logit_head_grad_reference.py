"""CPU: the checker of the logit head's own gradients (tests/logit_head_grad_reference.py).

* the float64 closed form equals torch autograd of HF's own OwlViTClassPredictionHead (live transformers, module in .double()) to 1e-12 relative to each
  gradient's largest element: per-image and shared banks, masks, both ELU branches;
* the simulation of the kernels sits inside the derived bounds on every shape of the GPU test, and every planted error leaves them;
* the C ABI's argument checks and workspace size (they run before any HIP call), and the host-side surface where no kernel is reached."""
import os
import types

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd import _lib, models, weights
from owl_vit_object_detection_amd.config import get_config
from tests import logit_head_grad_reference as H
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
    gen = torch.Generator().manual_seed(17)
    f = torch.randn(B, P, D, generator=gen, dtype=torch.float64)
    q = torch.randn(Q if shared else B * Q, Dt, generator=gen, dtype=torch.float64).view(*(() if shared else (B,)), Q, Dt)
    q = q * torch.logspace(-2, 1, Q, dtype=torch.float64)[:, None]
    mask = torch.rand(B, Q, generator=gen) > 0.3
    mask[:, 0] = True
    g = (0.1 * torch.randn(B, P, Q, generator=gen)).float()
    kept = {}
    hook = head.dense0.register_forward_hook(lambda m, i, o: kept.__setitem__("e", o))
    logits, _ = head(f, q[None].expand(B, -1, -1) if shared else q, mask)
    hook.remove()
    (logits * g.to(logits.dtype)).sum().backward()
    with torch.no_grad():
        shift = head.logit_shift(f).reshape(-1)
        scale = torch.nn.functional.elu(head.logit_scale(f)).reshape(-1) + 1.0
        assert bool((scale > 1.0).any()) and bool((scale <= 1.0).any()), "both ELU branches must occur in the inputs"
        r = R.exact_bwd(g, kept["e"].detach().reshape(B * P, Dt), q, shift, scale, head.logit_shift.weight, head.logit_scale.weight, B, P,
                        mask.to(torch.uint8), eps=1e-6)
        h = H.exact_head(r, f.reshape(B * P, D))
        hf = dict(dw_shift=head.logit_shift.weight.grad.reshape(-1), db_shift=head.logit_shift.bias.grad.reshape(()),
                  dw_scale=head.logit_scale.weight.grad.reshape(-1), db_scale=head.logit_scale.bias.grad.reshape(()))
        for k in H.KEYS:
            assert float(hf[k].abs().max()) > 0
            assert float((h[k] - hf[k]).abs().max()) <= 1e-12 * float(hf[k].abs().max()), k


VARIANTS = {"plain": {}, "shared": dict(shared=True, shared_mask=True), "underflow": dict(underflow=True), "poison": dict(poison=True)}
SIM = [(c, "plain") for c in H.GPU_CASES] + [(c, v) for c in (R.GPU_CASES[1], R.GPU_CASES[4]) for v in VARIANTS if v != "plain"]


@pytest.mark.parametrize("case,variant", SIM)
def test_simulation_sits_inside_the_bounds(case, variant):
    B, P, D = case[0], case[1], case[4]
    i = R.make_inputs(*case, seed=3, **VARIANTS[variant])
    r, h = H.exact_head_of(i, B, P)
    out = H.emulate_head_of(i, B, P)
    assert bool(torch.isfinite(out).all())
    b = H.bounds(r, h)
    worst = H.check_head(f"simulation {case} {variant}", out, r, h, b=b)
    # the bounds are tight enough to mean something: f32 round-off of the size of the terms summed (the sums themselves cancel: four rows can leave a
    # bias gradient a hundredth of its terms)
    absf = h["f"].abs()
    mag = dict(dw_shift=h["dsh"].abs() @ absf, dw_scale=h["ds"].abs() @ absf, db_shift=h["dsh"].abs().sum(), db_scale=h["ds"].abs().sum())
    rel = {k: float((b[k] / mag[k].clamp_min(1e-30)).max()) for k in H.KEYS}
    print(f"simulation {case} {variant}: err / tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + "; largest tol / sum |terms| "
          + " ".join(f"{k} {v:.1e}" for k, v in rel.items()))
    lim = 1e-3 if case[2] <= 70 else 5e-2          # (4096 queries: R's own limit for the inherited chain)
    assert max(rel.values()) < lim and max(worst.values()) <= 1.0


@pytest.mark.parametrize("hook", H.HOOKS)
def test_planted_errors_leave_the_bounds(hook):
    for case in (R.GPU_CASES[1], R.GPU_CASES[4], H.CHUNK_CASE):
        B, P = case[0], case[1]
        i = R.make_inputs(*case, seed=3)
        r, h = H.exact_head_of(i, B, P)
        fails = []
        H.check_head(f"{hook} {case}", H.emulate_head_of(i, B, P, hooks=(hook,)), r, h, fails)
        print(hook, case, [m.split(":")[0] for m in fails])
        assert fails, f"planted error `{hook}` passes the bounds on {case}"


def test_chunking_and_chain_lengths():
    assert H.CHUNK_CASE[1] > 2 * H.CHUNK and H.CHUNK_CASE[1] % H.CHUNK != 0          # several chunks, the last ragged
    assert H.n_sum64(2, 600) == 16 + 16 + 3 + 2 and H.n_sum64(3, 4) == 1 + 16 + 1 + 3 and H.n_sum64(32, 2304) == 16 + 16 + 9 + 32


def test_abi_argument_checks(built):
    nbytes, base = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    for want_dq in (0, 1):
        _lib.call("owl_class_logits_bwd_workspace_bytes", 2, 600, 5, 2, 64, want_dq, base)
        _lib.call("owl_class_logits_bwd_head_workspace_bytes", 2, 600, 5, 2, 64, 128, want_dq, nbytes)
        assert int(nbytes) == int(base) + 8 * 2 * 3 * (2 * 128 + 2)
    for args, word in (((3, 36, 0, 3, 192, 128, 1), "Q"), ((3, 36, 33, 3, 96, 128, 1), "Dt"), ((3, 8193, 33, 3, 192, 128, 1), "P"),
                       ((3, 36, 33, 2, 192, 128, 1), "nbanks"), ((3, 36, 33, 3, 192, 100, 1), "D %")):
        with pytest.raises(_lib.OwlLibError, match=word):
            _lib.call("owl_class_logits_bwd_head_workspace_bytes", *args, nbytes)
    with pytest.raises(_lib.OwlLibError, match="owl_class_logits_bwd_head: null pointer"):
        _lib.call("owl_class_logits_bwd_head", *([None] * 10), 0, *([None] * 8), 1, 4, 1, 1, 1, 64, 128)
    assert int(built.owl_abi_version()) == 8


def test_trainable_logit_head_on_the_host():
    """set_logit_head(trainable=True) where no kernel is reached: one flat buffer, four leaf views, the accessors, the frozen default."""
    cfg = get_config("tiny")
    D = cfg.hidden
    g = torch.Generator().manual_seed(4)
    good = {"logit_shift.weight": torch.randn(D, generator=g).numpy(), "logit_shift.bias": np.float32(0.5), "logit_scale.weight": torch.randn(D, generator=g),
            "logit_scale.bias": torch.tensor([0.25])}
    stub = types.SimpleNamespace(cfg=cfg, device_=torch.device("cpu"), logit_head=None)
    models.OwlViT.set_logit_head(stub, good)
    assert not any(t.requires_grad for t in stub.logit_head.values())
    assert models.OwlViT.logit_head_parameters(stub) == []          # a frozen head: nothing for an optimizer
    with pytest.raises(ValueError, match="empty parameter list"):
        torch.optim.AdamW(models.OwlViT.logit_head_parameters(stub))
    models.OwlViT.set_logit_head(stub, good, trainable=True)
    lh = stub.logit_head
    assert list(lh) == list(weights.LOGIT_HEAD_KEYS)
    leaves = models.OwlViT.logit_head_parameters(stub)
    assert [t.data_ptr() for t in leaves] == [lh[k].data_ptr() for k in weights.LOGIT_HEAD_KEYS]
    assert all(t.is_leaf and t.requires_grad and t.dtype == torch.float32 and t.dim() == 1 for t in leaves)
    flat = stub._logit_head_flat
    assert flat.shape == (2 * D + 2,) and not flat.requires_grad
    p0 = flat.data_ptr()
    assert [lh[k].data_ptr() - p0 for k in weights.LOGIT_HEAD_KEYS] == [0, 8 * D, 4 * D, 8 * D + 4]          # w_shift | w_scale | b_shift | b_scale
    assert torch.equal(flat[:D], torch.as_tensor(good["logit_shift.weight"])) and float(flat[2 * D]) == 0.5 and float(flat[2 * D + 1]) == 0.25
    # an optimizer of the caller's steps the shared storage in place
    opt = torch.optim.SGD(leaves, lr=1.0)
    for t in leaves:
        t.grad = torch.ones_like(t)
    before = flat.clone()
    opt.step()
    assert torch.equal(flat, before - 1.0)
    # logit_head_state: HF's shapes, numpy; it round-trips bitwise
    st = models.OwlViT.logit_head_state(stub)
    assert list(st) == list(weights.LOGIT_HEAD_KEYS) and st["logit_shift.weight"].shape == (D,) and st["logit_scale.bias"].shape == ()
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in st.values())
    models.OwlViT.set_logit_head(stub, st)
    assert not any(t.requires_grad for t in stub.logit_head.values())
    assert torch.equal(torch.cat([stub.logit_head[k] for k in ("logit_shift.weight", "logit_scale.weight", "logit_shift.bias", "logit_scale.bias")]), flat)
    models.OwlViT.set_logit_head(stub, None)
    assert stub.logit_head is None and models.OwlViT.logit_head_parameters(stub) == []
    with pytest.raises(RuntimeError, match="logit_head_state: no logit head"):
        models.OwlViT.logit_head_state(stub)
    import inspect
    sig = inspect.signature(models.load_model)
    assert sig.parameters["logit_head_trainable"].default is False and sig.parameters["logit_head_trainable"].kind is inspect.Parameter.KEYWORD_ONLY
