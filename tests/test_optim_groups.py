"""FusedAdamW with parameter groups, LR schedulers and gradient-norm clipping: the part that needs no GPU -- the three C-ABI entries (header,
dynamic symbol table, binding), their argument validation (it runs before any HIP call), the constructor's refusals and the torch LR schedulers
accepting the optimizer (a tiny model on the CPU: nothing is launched)."""
import ctypes
import os
import warnings

import pytest
import torch

from owl_vit_object_detection_amd import _lib, weights
from owl_vit_object_detection_amd.config import get_config
from owl_vit_object_detection_amd.models import OwlViT
from owl_vit_object_detection_amd.optim import FusedAdamW

ENTRIES = ("owl_grad_norm_workspace_bytes", "owl_grad_sumsq", "owl_adamw_step_grouped")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def model(built):
    cfg = get_config("tiny")
    return OwlViT(cfg, weights.make_weights(cfg), "cpu")


def _no_decay(model):
    """LayerNorm affines, biases and the query bank."""
    return [n for n in model.flat_offsets if n.endswith(".bias") or "layer_norm" in n or "layernorm" in n or n == "queries"]


def test_entries_in_header_map_and_binding(built):
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in protos and hasattr(lib, name) and name in _lib.protos(), name
        assert "_set_" not in name and "_debug" not in name
    assert _lib.header_abi_version() == 8 == built.owl_abi_version()           # purely additive: the version does not move
    assert protos["owl_grad_norm_workspace_bytes"][1] == [("int64_t", "n"), ("int64_t*", "bytes")]
    assert [a for _, a in protos["owl_grad_sumsq"][1]] == ["stream", "g", "n", "workspace"]
    step, grouped = [a for _, a in protos["owl_adamw_step"][1]], [a for _, a in protos["owl_adamw_step_grouped"][1]]
    assert grouped == step + ["seg_end", "seg_lr", "seg_wd", "nseg", "max_norm", "workspace", "norm_out"]
    assert protos["owl_adamw_step_grouped"][1][:len(step)] == protos["owl_adamw_step"][1]


def test_workspace_query_is_a_host_function(built):
    def q(n):
        b = torch.zeros(1, dtype=torch.int64)
        _lib.call("owl_grad_norm_workspace_bytes", n, b)
        return int(b.item())

    assert q(8) == 8 and q(1032) == 2 * 8                        # one f64 per workgroup of 256 float4
    assert q(1 << 20) == q(1 << 24) == q(1 << 33) > 0            # the grid is capped: a function of n alone
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_grad_norm_workspace_bytes", 8, None)
    with pytest.raises(_lib.OwlLibError, match="n % 4"):
        q(6)


def _grouped(n=16, seg_end=(8, 16), nseg=None, ptr=1 << 20, **over):
    """owl_adamw_step_grouped with made-up non-null device addresses: every case below is refused before any HIP call."""
    end = None if seg_end is None else torch.tensor(list(seg_end) + [0] * (40 - len(seg_end)), dtype=torch.int64)
    lr, wd = torch.full((40,), 1e-3), torch.zeros(40)
    a = dict(stream=None, p=ptr, g=ptr, m=ptr, v=ptr, p_bf16=None, n=n, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1,
             grad_scale=1.0, seg_end=end, seg_lr=lr, seg_wd=wd, nseg=nseg if nseg is not None else len(seg_end), max_norm=0.0, workspace=None,
             norm_out=None)
    a.update(over)
    assert list(a) == [name for _, name in _lib.parse_header()["owl_adamw_step_grouped"][1]]
    _lib.call("owl_adamw_step_grouped", *a.values())


@pytest.mark.parametrize("kw,msg", [
    (dict(nseg=0), r"1 <= nseg <= 32"),
    (dict(nseg=33, seg_end=tuple(range(4, 4 * 34, 4)), n=4 * 33), r"1 <= nseg <= 32"),
    (dict(seg_end=(8, 8)), r"strictly increasing"),
    (dict(seg_end=(12, 8, 16)), r"strictly increasing"),
    (dict(seg_end=(6, 16)), r"not a multiple of 4"),
    (dict(seg_end=(8, 12)), r"must equal n"),
    (dict(seg_end=(8, 20)), r"must equal n"),
    (dict(n=18, seg_end=(8, 18)), r"n % 4 == 0"),
    (dict(step=0), r"step >= 1"),
    (dict(p=None), r"null pointer"),
    (dict(g=None), r"null pointer"),
    (dict(m=None), r"null pointer"),
    (dict(v=None), r"null pointer"),
    (dict(seg_end=None, nseg=2), r"null pointer \(seg_end"),
    (dict(max_norm=1.0, workspace=None, norm_out=1 << 20), r"null pointer \(workspace, norm_out"),
    (dict(max_norm=1.0, workspace=1 << 20, norm_out=None), r"null pointer \(workspace, norm_out"),
])
def test_grouped_step_validation_names_the_rule(built, kw, msg):
    with pytest.raises(_lib.OwlLibError, match=msg):
        _grouped(**kw)
    assert "owl_adamw_step_grouped" in _lib.last_error()


def test_sumsq_validation(built):
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_grad_sumsq", None, None, 8, 1 << 20)
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_grad_sumsq", None, 1 << 20, 8, None)
    with pytest.raises(_lib.OwlLibError, match="n % 4"):
        _lib.call("owl_grad_sumsq", None, 1 << 20, 10, 1 << 20)


def test_constructor_surface_and_groups(model):
    opt = FusedAdamW(model, lr=3e-3, betas=(0.8, 0.9), eps=1e-7, weight_decay=0.1)
    assert isinstance(opt, torch.optim.Optimizer)
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay, opt.grad_scale, opt.step_count, opt.max_norm) == (3e-3, (0.8, 0.9), 1e-7, 0.1, 1.0, 0, None)
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == len(model.flat_offsets) == 29
    opt.lr = 1e-4
    assert opt.param_groups[0]["lr"] == 1e-4
    assert opt.last_grad_norm.shape == () and opt.last_grad_norm.dtype == torch.float32
    nd = _no_decay(model)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, param_groups=[dict(params=[model.p(n) for n in nd[:3]] + nd[3:], weight_decay=0.0, lr=5e-4)],
                     max_norm=2.0)
    g0, g1 = opt.param_groups
    assert (g0["lr"], g0["weight_decay"], g1["lr"], g1["weight_decay"]) == (1e-3, 0.1, 5e-4, 0.0) and opt.max_norm == 2.0
    assert {id(p) for p in g1["params"]} == {id(model.p(n)) for n in nd} and len(g0["params"]) + len(g1["params"]) == 29
    # runs of adjacent tensors of one group, in bucket order, ending where the next tensor starts (8-element aligned) and at the bucket's end
    ends = [e for e, _ in opt._segments]
    assert ends == sorted(set(ends)) and ends[-1] == model.flat_numel and all(e % 8 == 0 for e in ends) and len(ends) <= 32
    names = list(model.flat_offsets)
    for (end, gi), (prev, _) in zip(opt._segments, [(0, None)] + opt._segments):
        inside = [n for n in names if prev <= model.flat_offsets[n] < end]
        assert inside and all((n in nd) == (gi == 1) for n in inside)
    assert [gi for _, gi in opt._segments[:3]] == [1, 0, 1]                    # queries | q, k, v weights (merged) | q, k, v biases (merged)
    sd = opt.state_dict()
    assert {"step", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay"} <= set(sd)
    assert sd["max_norm"] == 2.0 and sd["groups"] == [dict(lr=1e-3, weight_decay=0.1), dict(lr=5e-4, weight_decay=0.0)]
    # every trainable tensor listed: no (empty) default group is left over
    assert len(FusedAdamW(model, param_groups=[dict(params=names, lr=1e-5)]).param_groups) == 1


class _ManyTensors(torch.nn.Module):
    """Just enough of the model's surface for the constructor's planning: 70 trainable tensors of 8 elements in one flat bucket."""

    def __init__(self, k=70):
        super().__init__()
        self.flat_param = torch.zeros(8 * k)
        self.flat_numel = 8 * k
        self.flat_offsets = {f"t{i}": 8 * i for i in range(k)}
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(self.flat_param[8 * i: 8 * i + 8]) for i in range(k)])

    def p(self, name):
        return self.ps[int(name[1:])]


def test_constructor_refusals_name_the_tensor(model):
    q, b = "queries", "box_head.dense2.bias"
    frozen = "backbone.pre_layernorm.weight"
    with pytest.raises(ValueError, match=f"`{q}` is in two parameter groups"):
        FusedAdamW(model, param_groups=[dict(params=[q, b]), dict(params=[model.p(q)])])
    with pytest.raises(ValueError, match=f"`{b}` is in two parameter groups"):
        FusedAdamW(model, param_groups=[dict(params=[b, b])])
    with pytest.raises(ValueError, match=f"`{frozen}`.*frozen"):
        FusedAdamW(model, param_groups=[dict(params=[frozen])])
    with pytest.raises(ValueError, match=f"`{frozen}`.*frozen"):
        FusedAdamW(model, param_groups=[dict(params=[model.p(frozen)])])
    with pytest.raises(ValueError, match=r"foreign tensor of shape \(3, 5\)"):
        FusedAdamW(model, param_groups=[dict(params=[torch.nn.Parameter(torch.zeros(3, 5))])])
    with pytest.raises(ValueError, match="`no.such.tensor`.*not a parameter"):
        FusedAdamW(model, param_groups=[dict(params=["no.such.tensor"])])
    with pytest.raises(ValueError, match=f"per-group `betas`.*`{q}`"):
        FusedAdamW(model, param_groups=[dict(params=[q], betas=(0.5, 0.9))])
    with pytest.raises(ValueError, match=f"per-group `eps`.*`{b}`"):
        FusedAdamW(model, param_groups=[dict(params=[b], eps=1e-3)])
    with pytest.raises(ValueError, match="max_norm"):
        FusedAdamW(model, max_norm=0.0)
    many = _ManyTensors()
    with pytest.raises(ValueError, match="more than 32 segments.*`t32`"):
        FusedAdamW(many, param_groups=[dict(params=[f"t{i}" for i in range(0, 70, 2)], weight_decay=0.0)])
    # the same tensors as neighbours merge into two segments
    assert len(FusedAdamW(many, param_groups=[dict(params=[f"t{i}" for i in range(35)], weight_decay=0.0)])._segments) == 2
    opt = FusedAdamW(model)
    with pytest.raises(ValueError, match="fixed at construction"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(8))]))


def test_torch_lr_schedulers_accept_and_drive_it(model):
    from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, LinearLR, SequentialLR
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, param_groups=[dict(params=_no_decay(model), weight_decay=0.0, lr=5e-4)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sched = LambdaLR(opt, lambda k: 0.5 ** k)
        assert sched.get_last_lr() == [1e-3, 5e-4]
        opt2 = FusedAdamW(model, lr=1e-3)
        lin = LinearLR(opt2, start_factor=0.25, end_factor=1.0, total_iters=3)
        assert opt2.lr == pytest.approx(2.5e-4) and lin.get_last_lr() == [opt2.lr]
        opt3 = FusedAdamW(model, lr=1e-3, param_groups=[dict(params=["queries"], lr=2e-3)])
        seq = SequentialLR(opt3, [LinearLR(opt3, start_factor=0.1, end_factor=1.0, total_iters=2), CosineAnnealingLR(opt3, T_max=4)], milestones=[2])
        assert [g["lr"] for g in opt3.param_groups] == pytest.approx([1e-4, 2e-4]) == seq.get_last_lr()
    assert [g["initial_lr"] for g in opt3.param_groups] == [1e-3, 2e-3]
    assert opt3.state_dict()["groups"][1] == dict(lr=pytest.approx(2e-4), weight_decay=0.01, initial_lr=2e-3)


def test_state_dict_loads_old_and_new_dicts(model):
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1, param_groups=[dict(params=["queries"], lr=2e-3, weight_decay=0.0)], max_norm=1.5)
    old = dict(step=7, exp_avg=torch.ones(model.flat_numel), exp_avg_sq=torch.full((model.flat_numel,), 2.0), lr=9.0, betas=(0.9, 0.999), eps=1e-8,
               weight_decay=0.5)                                       # the keys a dict written before the groups existed has
    opt.load_state_dict(old)
    assert opt.step_count == 7 and float(opt.exp_avg[5]) == 1.0 and float(opt.exp_avg_sq[-1]) == 2.0
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 2e-3] and opt.max_norm == 1.5          # untouched, as before
    new = dict(old, max_norm=None, groups=[dict(lr=1e-5, weight_decay=0.2, initial_lr=1e-3), dict(lr=2e-5, weight_decay=0.0, initial_lr=2e-3)])
    opt.load_state_dict(new)
    assert [(g["lr"], g["weight_decay"], g["initial_lr"]) for g in opt.param_groups] == [(1e-5, 0.2, 1e-3), (2e-5, 0.0, 2e-3)] and opt.max_norm is None
    with pytest.raises(ValueError, match="parameter groups"):
        opt.load_state_dict(dict(old, groups=[dict(lr=1.0)]))
