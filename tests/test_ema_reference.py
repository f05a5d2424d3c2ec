"""The EMA of the trainable bucket without a GPU: the float64 reference and its bound (tests/ema_reference.py) catch what they must, the decay rule's
closed forms, the C-ABI entries in header and binding, and the host side of FusedAdamW(ema_decay=) / ModelEMA on a CPU model (nothing is launched).

The checker against three wrong variants, 256 steps of a random-walk parameter (4096 elements, steps of 1e-3 around values of order 1), decay 0.999 with
warm-up -- the factor max |got - E| / B each one misses the bound by, as printed by test_wrong_variants_miss_the_bound:
    d and w swapped                       3.1e6
    warm-up ignored                       1.5e7
    update applied to the pre-step p      1.1e5
against at most 0.34 for the f32 emulation of the kernel's order (decay 0.999 and 0.9, warm-up on and off).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from owl_vit_object_detection_amd import _lib, optim, weights
from owl_vit_object_detection_amd.config import get_config
from owl_vit_object_detection_amd.models import OwlViT
from tests import ema_reference as R

STEPS, N = 256, 4096


def _walk(steps=STEPS, n=N, seed=0):
    """p_0 (the seed of the average) and p_1 .. p_T: f32 parameters of order 1 moving by steps of order 1e-3, like a trained tensor."""
    rng = np.random.default_rng(seed)
    p0 = p = rng.standard_normal(n).astype(np.float32)
    seq = []
    for _ in range(steps):
        p = (p + 1e-3 * rng.standard_normal(n)).astype(np.float32)
        seq.append(p)
    return p0, seq


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.999, 0.9])
def test_emulation_of_the_kernel_order_stays_inside_the_bound(decay, warmup):
    seed, seq = _walk()
    d, w = R.decays(STEPS, decay, warmup)
    E, B = R.recursion(seed, seq, d, w)
    f = R.miss_factor(R.emulate(seed, seq, d, w), E, B)
    print(f"decay {decay} warmup {warmup}: max |got - E| / B = {f:.3f}; max B / |E| = {float(np.max(B / np.maximum(np.abs(E), 1e-30))):.3e}")
    assert f <= 1.0
    assert float(np.median(B / np.abs(E))) < 1e-4          # the bound is a rounding-error bound, not a loose envelope


def test_wrong_variants_miss_the_bound():
    seed, seq = _walk()
    d, w = R.decays(STEPS, 0.999, True)
    E, B = R.recursion(seed, seq, d, w)
    flat_d, flat_w = R.decays(STEPS, 0.999, False)
    wrong = {
        "d and w swapped": R.emulate(seed, seq, w, d),
        "warm-up ignored": R.emulate(seed, seq, flat_d, flat_w),
        "update applied to the pre-step parameters": R.emulate(seed, [seed] + seq[:-1], d, w),
    }
    for what, got in wrong.items():
        f = R.miss_factor(got, E, B)
        print(f"{what}: misses the bound by a factor of {f:.3e}")
        assert f > 100.0, what


def test_bound_degenerate_decays():
    """d = 0: the average is fl(1 p) = p, exactly; d = 1: w = 0 and the average never moves.  The reference agrees and its bound stays a rounding bound."""
    seed, seq = _walk(steps=4)
    for decay, want in ((0.0, seq[-1]), (1.0, seed)):
        d, w = R.decays(4, decay, False)
        assert float(w[0]) == 1.0 - decay
        E, B = R.recursion(seed, seq, d, w)
        assert np.array_equal(E, want.astype(np.float64)) and np.array_equal(R.emulate(seed, seq, d, w), want)
        assert float(np.max(B / np.abs(E))) < 5 * R.U * 4


def test_decay_rule_closed_forms():
    assert optim.ema_decay_at(1, 0.999) == 2 / 11 == optim.ema_decay_at(1, 0.999, True)
    assert optim.ema_decay_at(1, 0.1) == 0.1                                    # a decay below the ramp is never raised
    # (1 + s) / (10 + s) >= 0.999  <=>  s >= 8990, where it is 8991 / 9000 = 0.999
    assert optim.ema_decay_at(8989, 0.999) == 8990 / 8999 < 0.999
    assert optim.ema_decay_at(8990, 0.999) == pytest.approx(0.999, abs=1e-15)
    assert optim.ema_decay_at(8991, 0.999) == 0.999 == optim.ema_decay_at(10 ** 9, 0.999)
    assert optim.ema_decay_at(1, 0.999, False) == 0.999 == optim.ema_decay_at(5000, 0.999, warmup=False)
    with pytest.raises(ValueError, match="1-based"):
        optim.ema_decay_at(0, 0.999)
    # the reference's closed form, written independently, and the coefficients the kernels are handed
    d, w = R.decays(9000, 0.999, True)
    for s in (1, 2, 10, 100, 8989, 8990, 8991, 9000):
        got = optim.ema_coefficients(optim.ema_decay_at(s, 0.999))
        assert got == (float(d[s - 1]), float(w[s - 1])), s
        assert np.float32(got[0]) == got[0] and np.float32(got[1]) == got[1]     # both are f32 values
    assert optim.ema_coefficients(0.0) == (0.0, 1.0) and optim.ema_coefficients(1.0) == (1.0, 0.0)


# ---- header, library, binding ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_entries_in_header_and_binding(built):
    protos = _lib.parse_header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("owl_ema_update", "owl_adamw_step_ema"):
        assert name in protos and hasattr(lib, name) and name in _lib.protos(), name
        assert getattr(built, name).argtypes == [_lib._CTYPES[t] for t, _ in protos[name][1]]
    assert _lib.header_abi_version() == 8 == built.owl_abi_version()           # purely additive: the version does not move
    assert protos["owl_ema_update"][1] == [("void*", "stream"), ("float*", "ema"), ("const float*", "p"), ("int64_t", "n"), ("float", "d"), ("float", "w")]
    assert protos["owl_adamw_step_ema"][1] == protos["owl_adamw_step_grouped"][1] + [("float*", "ema"), ("float", "d"), ("float", "w")]


def test_entry_validation_runs_before_any_launch(built):
    """Made-up non-null addresses: every case is refused before any HIP call."""
    ptr = 1 << 20
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        _lib.call("owl_ema_update", None, None, ptr, 8, 0.5, 0.5)
    with pytest.raises(_lib.OwlLibError, match="n % 4"):
        _lib.call("owl_ema_update", None, ptr, ptr, 6, 0.5, 0.5)
    step = lambda **kw: _lib.call("owl_adamw_step_ema", *dict(dict(stream=None, p=ptr, g=ptr, m=ptr, v=ptr, bf=None, n=16, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8,
                                                                   wd=0.1, step=1, gs=1.0, end=None, slr=None, swd=None, nseg=0, mn=0.0, ws=None, no=None,
                                                                   ema=ptr, d=0.5, w=0.5), **kw).values())
    with pytest.raises(_lib.OwlLibError, match="null pointer"):
        step(ema=None)
    with pytest.raises(_lib.OwlLibError, match="n % 4"):
        step(n=10)
    with pytest.raises(_lib.OwlLibError, match="must equal n"):
        step(end=torch.tensor([8], dtype=torch.int64), nseg=1)
    with pytest.raises(_lib.OwlLibError, match="workspace, norm_out"):
        step(mn=1.0)


# ---- the host side on a CPU model: nothing is launched ---------------------------------------------------------------------------------------------
@pytest.fixture()
def model(built):
    cfg = get_config("tiny")
    return OwlViT(cfg, weights.make_weights(cfg), "cpu")


def test_off_by_default_allocates_nothing(model):
    opt = optim.FusedAdamW(model, lr=1e-3)
    assert opt.ema is None and opt.ema_decay is None and opt.ema_updates == 0 and opt._ema_stash is None
    assert not {"ema", "ema_decay", "ema_warmup", "ema_updates"} & set(opt.state_dict())
    with pytest.raises(ValueError, match="ema_decay=None"):
        with opt.ema_weights():
            pass
    with pytest.raises(ValueError, match="ema_decay=None"):
        opt.ema_named()
    with pytest.raises(TypeError):
        optim.FusedAdamW(model, 1e-3, (0.9, 0.999), 1e-8, 1e-2, False, None, None, 0.9)          # keyword-only
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            optim.FusedAdamW(model, ema_decay=bad)
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            optim.ModelEMA(model, bad)


@pytest.mark.parametrize("kind", ["fused", "model_ema"])
def test_scope_swaps_and_restores_and_refuses(model, kind):
    holder = optim.FusedAdamW(model, lr=1e-3, ema_decay=0.9) if kind == "fused" else optim.ModelEMA(model, 0.9)
    assert torch.equal(holder.ema, model.flat_param) and holder.ema.data_ptr() != model.flat_param.data_ptr() and holder.ema_updates == 0
    views = holder.ema_named()
    assert list(views) == list(model.flat_offsets)
    for n, v in views.items():
        assert v.shape == model.p(n).shape and v.data_ptr() == holder.ema.data_ptr() + 4 * model.flat_offsets[n]
    with torch.no_grad():
        holder.ema.mul_(0.5)                           # an average that differs from the iterate
    raw, avg, ver = model.flat_param.clone(), holder.ema.clone(), model.flat_param._version
    frozen = {n: p.detach().clone() for n, p in model.named_parameters() if n not in model.flat_offsets}
    model._mark_bf16_current()                         # the token a fused step leaves
    with holder.ema_weights() as m:
        assert m is model and torch.equal(model.flat_param, avg) and model.flat_param._version > ver
        assert not (model._bf16_current and model._bf16_version == model.flat_param._version)          # void: the next forward recasts
        sd = model.state_dict()
        for n in model.flat_offsets:
            assert torch.equal(sd[n], views[n]), n
        with pytest.raises(RuntimeError, match="nested"):
            with holder.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside"):
            holder.load_state_dict(holder.state_dict())
        if kind == "fused":
            with pytest.raises(RuntimeError, match="inside"):
                holder.step()
            with pytest.raises(RuntimeError, match="inside"):
                holder.zero_grad()
        else:
            with pytest.raises(RuntimeError, match="inside"):
                holder.update()
        assert torch.equal(model.flat_param, avg)      # the refused calls changed nothing
    stash = holder._ema_stash
    assert torch.equal(model.flat_param, raw) and torch.equal(holder.ema, avg)
    assert not (model._bf16_current and model._bf16_version == model.flat_param._version)
    for n, p in model.named_parameters():
        if n in frozen:
            assert torch.equal(p, frozen[n]), n
    with pytest.raises(KeyError):                      # an exception inside the scope still restores the iterate
        with holder.ema_weights():
            raise KeyError("x")
    assert torch.equal(model.flat_param, raw) and holder._ema_stash is stash and not holder._ema_active


def test_state_dict_keys_and_reseeding(model):
    opt = optim.FusedAdamW(model, lr=1e-3, ema_decay=0.99, ema_warmup=False)
    with torch.no_grad():
        opt.ema.add_(1.0)
    opt.ema_updates = 7
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    assert sd["ema_decay"] == 0.99 and sd["ema_warmup"] is False and sd["ema_updates"] == 7 and torch.equal(sd["ema"], opt.ema)
    fresh = optim.FusedAdamW(model, lr=1e-3, ema_decay=0.5)
    fresh.load_state_dict(sd)
    assert fresh.ema_decay == 0.99 and fresh.ema_warmup is False and fresh.ema_updates == 7 and torch.equal(fresh.ema, sd["ema"])
    plain = {k: v for k, v in sd.items() if not k.startswith("ema")}
    fresh.load_state_dict(plain)                       # no average in the dict: re-seeded from the current parameters
    assert fresh.ema_updates == 0 and torch.equal(fresh.ema, model.flat_param) and fresh.ema_decay == 0.99
    none = optim.FusedAdamW(model, lr=1e-3)
    none.load_state_dict(sd)                           # an average in the dict, none kept here: ignored
    assert none.ema is None and none.ema_updates == 0 and none.ema_decay is None
    ema = optim.ModelEMA(model, 0.5)
    ema.load_state_dict(sd)
    assert ema.ema_updates == 7 and torch.equal(ema.ema, sd["ema"]) and set(ema.state_dict()) == {"ema", "ema_decay", "ema_warmup", "ema_updates"}
    ema.load_state_dict(plain)
    assert ema.ema_updates == 0 and torch.equal(ema.ema, model.flat_param)
