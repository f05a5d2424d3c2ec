"""Float64 reference, derived error bounds, inputs and an f32 simulation for OWLv2's objectness head: csrc/objectness.hip (objectness_final_rows_kernel<1/2>,
objectness_final_bwd_kernel and the slab reduces of gemm.hip behind it) and the head as a whole (two erf-GELU GEMMs + the tail).  Checker side;
device-agnostic: every function works on whatever device its inputs live on, and nothing here imports the package's Python ops.

Reference (float64 on the kernels' exact inputs: f32 values, bf16 values upcast)
---------
`head64(feats, head)`            HF's Owlv2BoxPredictionHead(out_dim=1): u0 = feats W0^T + b0, h0 = gelu(u0), u1 = h0 W1^T + b1, h1 = gelu(u1), o = h1 . w2 + b2
                                 (erf GELU).  tests/test_objectness_reference.py shows it equal to HF's module in .double() to 1e-12.
`head64_bwd(g, feats, head)`     the closed-form backward for an upstream g [rows]: du1 = g w2 gelu'(u1), dW1 = du1^T h0, db1 = sum du1, du0 = (du1 W1) gelu'(u0),
                                 dW0 = du0^T feats, db0 = sum du0, dw2 = g^T h1, db2 = sum g.  No gradient into feats: HF detaches them.
`exact_final(h, w2, b2)` / `exact_final_bwd(g, h1, u1, w2)`   the two tail kernels alone, on what they are GIVEN.
`model_tolerance(feats, head)`   fixture F20's per-element tolerance: the 1e-2 feature bar carried through the float64 head to first order, plus the two
                                 bf16 hidden layers' storage roundings carried the same way (torch autograd in double).

Bounds (elementwise, derived, no fitted constant; u, f, T, gamma(n), _V as tests/heads_reference.py uses them; contraction is OFF for objectness.hip,
so every written operation is one rounding and every fmaf one)
 forward (objectness.hip objectness_final_rows_kernel): a lane's chain is 8 NC fmaf (NC = 1 for D <= 512, else 2), the butterfly six levels:
     E_v = gamma(8 NC + 6) sum |h w|;  logits = fl(v + b2): one rounding.
 backward (objectness_final_bwd_kernel): dh1 = fl(g w), o = fl(dh1 dgelu_erf_f(u1)) with gemm_reference.dgelu_eval as dgelu_erf_f's evaluation error,
     du1 = bf16(o).  Row sums, counted as the source orders them: inside a workgroup rows in order: rpb steps (rpb = clamp(ceil(rows / 512), 8, 64)); dw2
     by fmaf (the product is not rounded), colsum by adds of the rounded o; db2: one row per thread (rpb <= 64 < 256), wave_sum (6), four waves in order
     (3); then owl_slab_reduce_impl over owl_objectness_final_bwd_blocks(rows) partials: heads_reference.n_reduce(nblk) (its count includes the add of an
     old value; these outputs are written, so the count is one above the chain):
         tol = gamma(n) sum_rows (|term| + E_term) + sum_rows E_term + T,    n = rpb + n_reduce (dw2, colsum),  9 + n_reduce (db2).
 head (`bounds_head`): gemm_reference's EPI_GELU bound for dense0 on the device's own feats; dense1 reads h0 within that bound: E_pre1 = E_h0 |W1|^T +
     gamma2(n_acc(D)) ((|h0| + E_h0) |W1|^T), the bias add, then EPI_GELU's output formula and the bf16 store; the tail reads h1 within E_h1:
     E_v = E_h1 |w2| + gamma(8 NC + 6) (|h1| + E_h1) |w2|.  The reference takes the bf16-rounded dense0 / dense1 weights: the GEMMs' exact operands.

`emulate_final` / `emulate_final_bwd` simulate the kernels in f32 in the order the source writes it and take `hooks` that plant errors; CPU test only,
NEVER a reference on the GPU.
"""
import torch

from tests.gemm_reference import (EPI_GELU, F, GELU_SUP2, TINY, U, _gelu_eval, bf16_round, bits, bounds as gemm_bounds, check, dgelu_erf_f32,  # noqa: F401
                                  dgelu_eval, exact as gemm_exact, gamma as gam, gamma2, gelu, gelu_d1, gelu_tanh, n_acc, ratios)
from tests.heads_reference import _slab_reduce, cdiv, n_reduce
from tests.layernorm_reference import _V, _fma32, _rnd, _wave_sum, padded, store_bf16  # noqa: F401

D_FEATS = 1e-2           # the bar tests/test_model_gpu.py asserts on an O(1) output of the bf16 trunk, per element of feats
KEYS = ("dense0.weight", "dense0.bias", "dense1.weight", "dense1.bias", "dense2.weight", "dense2.bias")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the launchers' choices, recomputed on the host
# ---------------------------------------------------------------------------------------------------------------------------------------------
def fwd_rpw(rows):                          # objectness.hip objectness_rpw
    return max(1, min(16, cdiv(rows, 4096)))


def bwd_rpb(rows):                          # objectness.hip objectness_bwd_rpb
    return max(8, min(64, cdiv(rows, 512)))


def bwd_blocks(rows):
    return cdiv(rows, bwd_rpb(rows))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _d(head):
    t = lambda v: torch.as_tensor(v).double()
    out = {k: t(head[k]) for k in KEYS}
    out["dense2.weight"] = out["dense2.weight"].reshape(-1)
    out["dense2.bias"] = out["dense2.bias"].reshape(())
    return out


def head64(feats, head, act=gelu):
    """feats [rows, D] (any float dtype) -> dict u0, h0, u1, h1, o (float64).  `act`: the activation (a planted error swaps it)."""
    w, f = _d(head), feats.double()
    u0 = f @ w["dense0.weight"].t() + w["dense0.bias"]
    h0 = act(u0)
    u1 = h0 @ w["dense1.weight"].t() + w["dense1.bias"]
    h1 = act(u1)
    return {"u0": u0, "h0": h0, "u1": u1, "h1": h1, "o": h1 @ w["dense2.weight"] + w["dense2.bias"]}


def head64_bwd(g, feats, head):
    """-> {key: float64 gradient} in HF's shapes ([D, D], [D], [D, D], [D], [D], 0-d) for the upstream g [rows]."""
    w, r, g, f = _d(head), head64(feats, head), g.double().reshape(-1), feats.double()
    du1 = g[:, None] * w["dense2.weight"][None] * gelu_d1(r["u1"])
    du0 = (du1 @ w["dense1.weight"]) * gelu_d1(r["u0"])
    return {"dense0.weight": du0.t() @ f, "dense0.bias": du0.sum(0), "dense1.weight": du1.t() @ r["h0"], "dense1.bias": du1.sum(0),
            "dense2.weight": g @ r["h1"], "dense2.bias": g.sum()}


def model_tolerance(feats, head, d_feats=D_FEATS):
    """tol[row] = d_feats ||d o / d feats[row]||_1 + u sum_j |h0_j| |d o / d h0_j| + u sum_j |h1_j| |d o / d h1_j| in float64 by torch autograd (a row of o
    depends on its own row of feats alone, so one backward of o.sum() gives every row's gradient)."""
    w = _d(head)
    f = feats.double().clone().requires_grad_(True)
    h0 = gelu(f @ w["dense0.weight"].t() + w["dense0.bias"])
    h0.retain_grad()
    h1 = gelu(h0 @ w["dense1.weight"].t() + w["dense1.bias"])
    h1.retain_grad()
    (h1 @ w["dense2.weight"] + w["dense2.bias"]).sum().backward()
    return (d_feats * f.grad.abs().sum(-1) + U * (h0.detach().abs() * h0.grad.abs()).sum(-1) + U * (h1.detach().abs() * h1.grad.abs()).sum(-1)).detach()


def exact_final(h, w2, b2):
    hd, wd = h.double(), w2.double().reshape(-1)
    v = hd @ wd
    return {"v": v, "v_abs": hd.abs() @ wd.abs(), "logits": v + b2.double().reshape(()), "D": hd.shape[1]}


def exact_final_bwd(g, h1, u1, w2):
    g, h, u, w = g.double().reshape(-1), h1.double(), u1.double(), w2.double().reshape(-1)
    du1 = g[:, None] * w[None] * gelu_d1(u)
    return {"du1": du1, "dw2": g @ h, "db2": g.sum(), "colsum": du1.sum(0), "in": {"g": g, "h": h, "u": u, "w": w}}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _nc(D):
    return 1 if D <= 512 else 2


def bounds_final(r):
    E_v = gam(8 * _nc(r["D"]) + 6) * r["v_abs"] + TINY
    return {"logits": _rnd(r["logits"], E_v) + TINY}


def bounds_final_bwd(x):
    i = x["in"]
    rows, D = i["h"].shape
    G, Wk = _V(i["g"][:, None]), _V(i["w"][None])
    o = (G * Wk) * _V(gelu_d1(i["u"]), dgelu_eval(i["u"]))
    rpb, nr = bwd_rpb(rows), n_reduce(bwd_blocks(rows))
    gh = (i["g"][:, None] * i["h"]).abs().sum(0)
    return {"du1": store_bf16(x["du1"], o.E), "dw2": gam(rpb + nr) * gh + TINY, "db2": gam(9 + nr) * i["g"].abs().sum() + TINY,
            "colsum": gam(rpb + nr) * (o.v.abs() + o.E).sum(0) + o.E.sum(0) + TINY}


def bounds_head(feats, head):
    """The whole head on the device: feats = the bf16 values it read; head = its f32 tensors.  -> (reference dict of head64 at the bf16-rounded dense0 /
    dense1 weights, tol [rows] for the logits)."""
    w = _d(head)
    W0, W1 = bf16_round(w["dense0.weight"].float()).double(), bf16_round(w["dense1.weight"].float()).double()
    ref = head64(feats, dict(head, **{"dense0.weight": W0, "dense1.weight": W1}))
    r0 = gemm_exact(EPI_GELU, feats, W0, bias=w["dense0.bias"])
    E_h0 = gemm_bounds(r0)["out"]
    h0, K = ref["h0"], W1.shape[1]
    acc, mag = h0 @ W1.t(), (h0.abs() + E_h0) @ W1.abs().t()
    E = E_h0 @ W1.abs().t() + gamma2(n_acc(K)) * mag
    E = E + F * (acc.abs() + E)
    E = E + F * (ref["u1"].abs() + E) + TINY
    Eo = gelu_d1(ref["u1"]).abs() * E + 0.5 * GELU_SUP2 * E * E + _gelu_eval(ref["u1"]) + 1.2 * E * 16.0 * F
    E_h1 = store_bf16(ref["h1"], Eo)
    w2 = w["dense2.weight"].abs()
    E_v = E_h1 @ w2 + gam(8 * _nc(K) + 6) * ((ref["h1"].abs() + E_h1) @ w2)
    return ref, _rnd(ref["o"], E_v) + TINY


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _gen(seed, rows, D):
    return torch.Generator(device="cpu").manual_seed(seed * 1000003 + rows * 10007 + D * 101 + 20)


def make_inputs(rows, D, seed=0, profile="randn"):
    """Tail inputs on the CPU: u1 / h1 (float32 holding bf16 values, h1 = gelu(u1)), w2 [D], b2 [1], g [rows] (mixed signs; g[0] < 0).
    profile "saturated": u1 at +-30, where GELU' is exactly 0 or 1."""
    gn = _gen(seed, rows, D)
    u1 = bf16_round(2.0 * torch.randn(rows, D, generator=gn))
    if profile == "saturated":
        u1 = torch.where(torch.rand(rows, D, generator=gn) < 0.5, -30.0, 30.0)
    h1 = bf16_round(torch.nn.functional.gelu(u1))
    w2 = 0.1 * torch.randn(D, generator=gn)
    b2 = torch.tensor([-1.0]) + 0.1 * torch.randn(1, generator=gn)
    g = torch.randn(rows, generator=gn)
    g[0] = -g[0].abs() - 0.1
    return {"h1": h1, "u1": u1, "w2": w2.float(), "b2": b2.float(), "g": g.float()}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def emulate_final(h, w2, b2, hooks=()):
    """objectness_final_rows_kernel -> logits.  hooks: "no_b2", "bf16_acc" (the chain rounded to bf16 after every step), "chunk_alias" (the second
    512-column chunk multiplies by the first chunk's weights)."""
    h, w2 = h.float(), w2.float().reshape(-1)
    R_, D = h.shape
    NC = _nc(D)
    buf_h, buf_w = torch.zeros(R_, 512 * NC), torch.zeros(512 * NC)
    buf_h[:, :D], buf_w[:D] = h, w2
    hh, ww = buf_h.view(R_, NC, 64, 8), buf_w.view(NC, 64, 8)
    a = torch.zeros(R_, 64)
    for c in range(NC):
        cw = 0 if "chunk_alias" in hooks else c
        for k in range(8):
            a = _fma32(hh[:, c, :, k], ww[None, cw, :, k], a)
            if "bf16_acc" in hooks:
                a = bf16_round(a)
    v = _wave_sum(a, [0])[:, 0]
    return v if "no_b2" in hooks else v + b2.float().reshape(())


def _dgelu_tanh_f32(u):
    u = u.double().clone().requires_grad_(True)
    gelu_tanh(u).sum().backward()
    return u.grad.float()


def emulate_final_bwd(g, h1, u1, w2, hooks=(), guard=None):
    """objectness_final_bwd_kernel + the slab reduces -> du1 (bf16 values), dw2, db2, colsum.  hooks: "tanh_dgelu", "dgelu_at_h1", "dw2_from_u1", "db2_abs"
    (the sign of g lost), "db2_last" (no sum: the last row alone), "row_past" (the row behind `rows` -- `guard` = (g, h1, u1) of that row -- summed in),
    "drop_ragged_block" (a last workgroup with fewer than rpb rows writes no partial)."""
    g, h, u, w = g.float().reshape(-1), h1.float(), u1.float(), w2.float().reshape(-1)
    if "row_past" in hooks:
        g, h, u = torch.cat([g, guard[0].float().reshape(1)]), torch.cat([h, guard[1].float()[None]]), torch.cat([u, guard[2].float()[None]])
    R_, D = h.shape
    rows = R_ - (1 if "row_past" in hooks else 0)
    dg = _dgelu_tanh_f32(u) if "tanh_dgelu" in hooks else dgelu_erf_f32(h if "dgelu_at_h1" in hooks else u)
    o = (g[:, None] * w[None]) * dg
    rpb, nblk = bwd_rpb(rows), bwd_blocks(rows)
    nb_all = max(nblk, cdiv(R_, rpb))

    def blocks(t):
        buf = torch.zeros(nb_all * rpb, *t.shape[1:])
        buf[:R_] = t
        return buf.view(nb_all, rpb, *t.shape[1:])

    src = u if "dw2_from_u1" in hooks else h
    bg, bs, bo = blocks(g), blocks(src), blocks(o)
    pw, po = torch.zeros(nb_all, D), torch.zeros(nb_all, D)
    for i in range(rpb):
        pw, po = _fma32(bg[:, i, None], bs[:, i], pw), po + bo[:, i]
    lanes = torch.zeros(nb_all, 64)
    lanes[:, :rpb] = bg.abs() if "db2_abs" in hooks else bg
    pb = _wave_sum(lanes, [0])[:, :1]
    if "db2_last" in hooks:
        pb = torch.zeros(nb_all, 1)
        pb[-1, 0] = g[-1]
    if nb_all > nblk:          # (row_past opened a workgroup of its own: it belongs to the last real one's sums)
        pw[nblk - 1], po[nblk - 1], pb[nblk - 1] = pw[nblk - 1] + pw[nblk], po[nblk - 1] + po[nblk], pb[nblk - 1] + pb[nblk]
        pw, po, pb = pw[:nblk], po[:nblk], pb[:nblk]
    if "drop_ragged_block" in hooks and rows % rpb:
        pw[-1], po[-1], pb[-1] = 0.0, 0.0, 0.0
    z = lambda n: torch.zeros(n)
    return {"du1": bf16_round(o[:rows]), "dw2": _slab_reduce(pw, z(D)), "db2": _slab_reduce(pb, z(1))[0], "colsum": _slab_reduce(po, z(D))}


FWD_HOOKS = ("no_b2", "bf16_acc", "chunk_alias")
BWD_HOOKS = ("tanh_dgelu", "dgelu_at_h1", "dw2_from_u1", "db2_abs", "db2_last", "row_past", "drop_ragged_block")


def hook_applies(hook, rows, D):
    """Where a planted error can show at all: the second chunk exists, the sum has more than one term, the last workgroup is ragged."""
    if hook == "chunk_alias":
        return D > 512
    if hook == "db2_last":
        return rows > 1
    if hook == "drop_ragged_block":
        return rows % bwd_rpb(rows) != 0
    return True


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case set of the GPU test: the issue's shapes, plus one at which a wave walks more than one row (rpw 2) and the backward has several workgroups and a
# ragged last one (4100 = 455 x 9 + 5); (1, 8) and (3, 128) are single ragged workgroups, (65, 512) has nine with one row in the last
# ---------------------------------------------------------------------------------------------------------------------------------------------
CASES = ((1, 8), (3, 128), (37, 128), (108, 128), (65, 512), (5, 520), (4, 768), (9, 1024), (4100, 128), (16, 128))
