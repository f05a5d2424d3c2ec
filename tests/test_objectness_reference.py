"""CPU: tests/objectness_reference.py is what it says -- the float64 head equals HF's Owlv2BoxPredictionHead(out_dim=1) in .double() and its autograd, and
fixture F20 at f32 round-off; the f32 simulation of the two tail kernels sits inside the derived bounds on every GPU case's inputs, and every planted
error misses them there; the case set reaches every launcher form the issue names."""
import os

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd.config import get_config
from tests import objectness_reference as R
from tests.golden.make_golden_objectness import KEYS, objectness_head, target


class _HFHead(torch.nn.Module):
    """Owlv2BoxPredictionHead(out_dim=1) as transformers/models/owlv2/modeling_owlv2.py writes it: three Linear layers, nn.GELU() between them."""

    def __init__(self, D):
        super().__init__()
        self.dense0, self.dense1, self.dense2, self.gelu = torch.nn.Linear(D, D), torch.nn.Linear(D, D), torch.nn.Linear(D, 1), torch.nn.GELU()

    def forward(self, feats):
        return self.dense2(self.gelu(self.dense1(self.gelu(self.dense0(feats.detach())))))[..., 0]


@pytest.fixture(scope="module")
def f20(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f20_owlv2_objectness.npz")))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_head64_and_its_closed_form_backward_equal_the_module_in_double():
    D, rows = 24, 13
    g = torch.Generator().manual_seed(1)
    m = _HFHead(D).double()
    for p in m.parameters():
        p.data = 0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64)
    head = {k: dict(m.named_parameters())[k].detach() for k in KEYS}
    feats = torch.randn(rows, D, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(rows, generator=g, dtype=torch.float64)
    o = m(feats)
    assert _rel(R.head64(feats.detach(), head)["o"], o.detach()) < 1e-12
    (o * up).sum().backward()
    assert feats.grad is None          # the head reads its input detached
    got = R.head64_bwd(up, feats.detach(), head)
    for k, p in m.named_parameters():
        assert _rel(got[k].reshape(p.shape), p.grad) < 1e-12, k
    # the tail kernels' closed forms are the same expressions on what they are given
    r = R.head64(feats.detach(), head)
    x = R.exact_final_bwd(up, r["h1"], r["u1"], head["dense2.weight"])
    assert _rel(x["dw2"], got["dense2.weight"]) < 1e-12 and _rel(x["colsum"], got["dense1.bias"]) < 1e-12 and _rel(x["db2"].reshape(1), got["dense2.bias"].reshape(1)) < 1e-12
    assert _rel(R.exact_final(r["h1"], head["dense2.weight"], head["dense2.bias"])["logits"], o.detach()) < 1e-12


def test_fixture_is_the_float64_head_at_f32_roundoff(f20):
    cfg = get_config("tiny")
    head = objectness_head(cfg, int(f20["head_seed"]))
    B, P, D = f20["feats"].shape
    feats = torch.from_numpy(f20["feats"]).reshape(B * P, D)
    o = R.head64(feats, head)["o"].reshape(B, P)
    assert float((torch.from_numpy(f20["objectness_logits"]).double() - o).abs().max()) < 2e-6
    t = torch.from_numpy(f20["target"])
    assert np.array_equal(f20["target"], target(cfg)) and 0 < float(t.mean()) < 0.5
    g = (torch.sigmoid(o) - t.double()) / B          # d/do of BCE-with-logits, reduction sum, / 3
    got = R.head64_bwd(g.reshape(-1), feats, head)
    for k in KEYS:
        ref = torch.from_numpy(f20["grad/" + k]).double()
        assert _rel(got[k].reshape(ref.shape), ref) < 1e-5, k
    # the tolerance is the stored construction, and it decides every image's arg-max patch
    tol = R.model_tolerance(feats, head).reshape(B, P)
    assert float((tol - torch.from_numpy(f20["tol"]).double()).abs().max()) < 1e-9
    top = torch.topk(o, 2, dim=1)
    assert bool((top.values[:, 0] - top.values[:, 1] > tol.gather(1, top.indices).sum(1)).all())
    print(f"F20: tol {float(tol.min()):.3f} .. {float(tol.max()):.3f}, logit spread {float(o.max() - o.min()):.3f}")


def test_quick_gelu_in_the_head_misses_the_gradient_band(f20):
    """The planted model-level error: the trunk's activation in the head, on the model case's inputs (F20).  Where it shows is the GRADIENT check: the six
    gradients of the fixture's loss under quick-GELU sit outside the end-to-end band the GPU test holds the device to (rel-L2 <= 2e-2): dense0.weight
    3.0e-2, dense0.bias 2.6e-2, dense1.weight 2.1e-2.  Against HF's LOGITS at F20's stored tolerance it does NOT show, and that is recorded, not hidden:
    the tolerance is the trunk's 1e-2 feature bar carried through the head (0.04 .. 0.08) and quick-GELU moves these logits by at most 0.022, err / tol
    0.37; a worst-case bound through two 128-wide layers is wider still.  The two activations differ by at most 0.02 per hidden unit and the differences
    add like a random walk, the bounds add linearly."""
    cfg = get_config("tiny")
    head = objectness_head(cfg, int(f20["head_seed"]))
    B, P, D = f20["feats"].shape
    feats = torch.from_numpy(f20["feats"]).reshape(B * P, D).double()
    w = {k: torch.from_numpy(np.asarray(head[k])).double().requires_grad_(True) for k in KEYS}
    q = lambda x: x * torch.sigmoid(1.702 * x)
    o = q(q(feats @ w["dense0.weight"].t() + w["dense0.bias"]) @ w["dense1.weight"].t() + w["dense1.bias"]) @ w["dense2.weight"] + w["dense2.bias"]
    t = torch.from_numpy(f20["target"]).double().reshape(-1)
    (torch.nn.functional.binary_cross_entropy_with_logits(o, t, reduction="sum") / B).backward()
    rel = {}
    for k in KEYS:
        r, g = torch.from_numpy(f20["grad/" + k]).double().reshape(-1), w[k].grad.reshape(-1)
        rel[k] = float((g - r).norm() / r.norm())
    vs_hf = (o.detach().reshape(B, P) - torch.from_numpy(f20["objectness_logits"]).double()).abs() / torch.from_numpy(f20["tol"]).double()
    print("quick-GELU in the head: gradient rel-L2 " + ", ".join(f"{k} {v:.2e}" for k, v in rel.items()) + f"; logits err / tol {float(vs_hf.max()):.2f}")
    assert max(rel.values()) > 2e-2 and sum(v > 2e-2 for v in rel.values()) >= 3


def test_case_set_reaches_every_launcher_form():
    rows = [r for r, _ in R.CASES]
    assert max(R.fwd_rpw(r) for r in rows) > 1                                                   # a wave walks more than one row
    assert any(D <= 512 for _, D in R.CASES) and any(D > 512 and D % 512 for _, D in R.CASES) and any(D == 1024 for _, D in R.CASES)
    blocks = {r: R.bwd_blocks(r) for r in rows}
    assert any(b == 1 for b in blocks.values()) and any(b > 1 for b in blocks.values())
    assert any(b > 1 and r % R.bwd_rpb(r) for r, b in blocks.items()) and any(r % R.bwd_rpb(r) == 0 for r in rows)      # a ragged last workgroup, and a full one
    assert any(b >= 128 for b in blocks.values()) and any(1 < b < 128 for b in blocks.values())   # both reducers of owl_slab_reduce_impl
    for h in R.FWD_HOOKS + R.BWD_HOOKS:
        assert any(R.hook_applies(h, r, D) for r, D in R.CASES), h


@pytest.mark.parametrize("rows,D", R.CASES)
def test_emulation_inside_the_bounds_and_planted_errors_outside(rows, D):
    for profile in ("randn", "saturated"):
        x = R.make_inputs(rows, D, profile=profile)
        rf = R.exact_final(x["h1"], x["w2"], x["b2"])
        worst = R.check(f"fwd {rows}x{D} {profile}", R.emulate_final(x["h1"], x["w2"], x["b2"]), rf["logits"], R.bounds_final(rf)["logits"])
        rb = R.exact_final_bwd(x["g"], x["h1"], x["u1"], x["w2"])
        tb = R.bounds_final_bwd(rb)
        got = R.emulate_final_bwd(x["g"], x["h1"], x["u1"], x["w2"])
        for k in ("du1", "dw2", "db2", "colsum"):
            worst = max(worst, R.check(f"bwd {k} {rows}x{D} {profile}", got[k], rb[k], tb[k]))
        assert worst <= 1.0
    x = R.make_inputs(rows, D)
    rf, rb = R.exact_final(x["h1"], x["w2"], x["b2"]), R.exact_final_bwd(x["g"], x["h1"], x["u1"], x["w2"])
    tf, tb = R.bounds_final(rf), R.bounds_final_bwd(rb)
    for hook in R.FWD_HOOKS:
        if R.hook_applies(hook, rows, D):
            fails = []
            R.check(hook, R.emulate_final(x["h1"], x["w2"], x["b2"], hooks=(hook,)), rf["logits"], tf["logits"], fails)
            assert fails, f"planted error `{hook}` stays inside the bound at {rows} x {D}"
    guard = (torch.tensor(1.5), torch.ones(D), torch.ones(D))
    for hook in R.BWD_HOOKS:
        if R.hook_applies(hook, rows, D):
            fails = []
            got = R.emulate_final_bwd(x["g"], x["h1"], x["u1"], x["w2"], hooks=(hook,), guard=guard)
            for k in ("du1", "dw2", "db2", "colsum"):
                R.check(f"{hook} {k}", got[k], rb[k], tb[k], fails)
            assert fails, f"planted error `{hook}` stays inside every bound at {rows} x {D}"


def test_bounds_head_holds_an_f32_chain():
    """The composite bound on a CPU stand-in for the device's chain: bf16 weights and hidden layers, f32 arithmetic."""
    cfg = get_config("tiny")
    head = objectness_head(cfg, 7)
    g = torch.Generator().manual_seed(3)
    feats = R.bf16_round(torch.randn(50, cfg.hidden, generator=g))
    ref, tol = R.bounds_head(feats, head)
    W0, W1 = R.bf16_round(torch.from_numpy(head["dense0.weight"])), R.bf16_round(torch.from_numpy(head["dense1.weight"]))
    F_ = torch.nn.functional
    h0 = R.bf16_round(F_.gelu(feats @ W0.t() + torch.from_numpy(head["dense0.bias"])))
    h1 = R.bf16_round(F_.gelu(h0 @ W1.t() + torch.from_numpy(head["dense1.bias"])))
    o = R.emulate_final(h1, torch.from_numpy(head["dense2.weight"]), torch.tensor([float(head["dense2.bias"])]))
    assert R.check("head chain", o, ref["o"], tol) <= 1.0
