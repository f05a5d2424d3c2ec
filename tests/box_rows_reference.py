"""Float64 restatement of the box head's backward on the rows that carry a gradient (csrc/box_rows_bwd.hip + the compact products of
autograd.backward_impl), with derived bounds.  Checker side: numpy for the compaction, float64 torch for the gradients; works on whatever device its
inputs live on.  The conventions (u, f, gamma, gamma2, n_acc, T) are tests/gemm_reference.py's, the tail's per-row error terms tests/heads_reference.py's.

Compaction (`compact`)
----------------------
row r of dboxes [rows, 4] is listed iff one of its components is not == 0 (NaN and inf are listed, -0.0 is zero); the list is ascending; at most `cap`
entries are kept and `overflow` says that more rows were non-zero.

The six gradients over a row list (`exact_six`), L = the listed rows in list order:
    dlin = (g0 + g2, g1 + g3, (g2 - g0) / 2, (g3 - g1) / 2),  dpre = dlin s (1 - s)                      (heads_reference.exact_box_final_bwd)
    o    = (dpre W2) gelu'(ub1),   du1 = bf16(o)                      dense2.weight = dpre^T hb1,  dense2.bias = sum_L dpre,  dense1.bias = sum_L o
    du0  = bf16((du1 W1) gelu'(ub0))                                   dense1.weight = du1^T hb0
                                                                       dense0.weight = du0^T feats, dense0.bias = sum_L du0
The device rounds du1 and du0 to bf16 before the products read them; a test on the device passes the du1 / du0 the path under test left (`given_du1`,
`given_du0`, bf16-exact) so that the three sums over them are held as SUMS, not through the roundings of their operands (du1 itself is held bit for
bit to the dense kernel and through heads_reference's bound).

Bounds (`bounds_six`; elementwise, no fitted constant)
------------------------------------------------------
The row path keeps the dense launches' grouping and order of every sum (the tail groups the listed rows as box_final_bwd_kernel groups all rows and its
reduce walks the groups as owl_slab_reduce_impl walks the workgroup partials; the two weight-gradient products ARE the dense launches, on operands that
are zero outside the list), so one set of bounds at the dense row count R = B P holds both paths -- and the GPU test holds them to each other bit for bit.
 dense2.weight, dense2.bias, dense1.bias: heads_reference.bounds_box_final_bwd's formulas on the listed rows (a zero row adds exact zeros):
       tol = gamma(n) (sum_L (|term| + E_term) + |old|) + sum_L E_term + T,   n = rpb + n_reduce(blocks) (dW2, column sums), 9 + n_reduce (db2)
 dense1.weight, dense0.weight: products of bf16-exact operands are exact; the MFMAs of either route (TN split-K, gemm_tn.hip; NT split-K through the
   transposes) add them in f32 with every add budgeted at 2 f (ASSUMPTION 1 of gemm_reference.py): a product passes at most n_acc(Kp) adds inside its
   split, Kp = R rounded up to the 64-row K-tiles, and the slab reduce adds at most ns + 1 <= 257 values (dw_reference.py, `tol_w`):
       tol = gamma2(n_acc(Kp) + 257) sum_L |dy| |x| + Kp T
 dense0.bias: the TN kernel's fold (dw_reference.py: 32 adds per K-tile at 2 f each, one join) or the transposing column sum (64 + 16 adds), then
   the reduce:     tol = gamma2(32 ceil(Kp / 64) + 1 + 257) sum_L |du0| + Kp T
"""
import numpy as np
import torch

from tests import heads_reference as H
from tests.gemm_reference import F, TINY, bf16_round, gamma, gamma2, gelu_d1, n_acc  # noqa: F401
from tests.layernorm_reference import _V, store_bf16

RPB = 8          # the compact operands' row count is a multiple of 8
SIX = ("dense2.weight", "dense2.bias", "dense1.weight", "dense1.bias", "dense0.weight", "dense0.bias")


def cap_pad(cap):
    return (max(int(cap), 1) + RPB - 1) // RPB * RPB


def compact(dboxes, cap):
    """-> (row_list int32 [count], count, overflow)."""
    g = np.asarray(dboxes, dtype=np.float32).reshape(-1, 4)
    nz = np.nonzero(~(g == 0).all(axis=1))[0]          # NaN == 0 is False: listed
    return nz[:cap].astype(np.int32), int(min(len(nz), cap)), bool(len(nz) > cap)


def exact_six(dboxes, sig, hb1, ub1, hb0, ub0, feats, w2, w1, rows, given_du1=None, given_du0=None):
    """float64 reference over the row list `rows` (module docstring).  dboxes / sig f32 [R, 4]; hb1, ub1, hb0, ub0, feats bf16-exact [R, D]; w2 f32 [4, D];
    w1 [D, D] (out, in) as the GEMM reads it (bf16-exact).  -> dict: the six gradients, their `abs` sums, du1 / du0 (what the products read), and
    `tail`: heads_reference.exact_box_final_bwd on the listed rows."""
    idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=dboxes.device)
    L = lambda t: t[idx]
    tail = H.exact_box_final_bwd(L(dboxes), L(sig), L(hb1), L(ub1), w2)
    du1 = bf16_round(tail["du1"]) if given_du1 is None else given_du1.double()
    if given_du0 is None:
        du0 = bf16_round((du1 @ w1.double()) * gelu_d1(L(ub0).double()))
    else:
        du0 = given_du0.double()
    h0, ft = L(hb0).double(), L(feats).double()
    g = {"dense2.weight": tail["dW2"], "dense2.bias": tail["db2"], "dense1.bias": tail["colsum"], "dense1.weight": du1.t() @ h0,
         "dense0.weight": du0.t() @ ft, "dense0.bias": du0.sum(0)}
    a = {"dense1.weight": du1.abs().t() @ h0.abs(), "dense0.weight": du0.abs().t() @ ft.abs(), "dense0.bias": du0.abs().sum(0)}
    return {"grads": g, "abs": a, "du1": du1, "du0": du0, "tail": tail, "n": len(idx)}


OLD_KEY = {"dense2.weight": "dW2", "dense2.bias": "db2", "dense1.bias": "colsum"}          # heads_reference's names of what the tail accumulates into


def _tail_bounds(x, chain_w, chain_b, old=None):
    """heads_reference.bounds_box_final_bwd's formulas on the listed rows, with the dense kernel's chain lengths at the DENSE row count (the caller's)."""
    old = old or {}
    ov = lambda k: old[k].double().abs() if k in old else 0.0
    i = x["in"]
    G, S = [_V(i["g"][:, k:k + 1]) for k in range(4)], [_V(i["s"][:, k:k + 1]) for k in range(4)]
    half = lambda t: _V(0.5 * t.v, 0.5 * t.E)
    dl = [G[0] + G[2], G[1] + G[3], half(G[2] - G[0]), half(G[3] - G[1])]
    one = _V(torch.ones_like(S[0].v))
    dp = [(dl[k] * S[k]) * (one - S[k]) for k in range(4)]
    Wk = [_V(i["w"][k:k + 1]) for k in range(4)]
    dh1 = ((dp[0] * Wk[0] + dp[1] * Wk[1]) + dp[2] * Wk[2]) + dp[3] * Wk[3]
    o = dh1 * _V(H.gelu_d1(i["u"]), H.dgelu_eval(i["u"]))
    Hh = _V(i["h"])
    red = lambda t, n, o_=0.0: gamma(n) * ((t.v.abs() + t.E).sum(0) + o_) + t.E.sum(0) + TINY
    ow = old.get("dW2")
    dW2 = torch.stack([red(dp[k] * Hh, chain_w, ow[k].double().abs() if ow is not None else 0.0) for k in range(4)])
    dpv = _V(torch.cat([t.v for t in dp], 1), torch.cat([t.E for t in dp], 1))
    return {"du1": store_bf16(x["du1"], o.E), "dense2.weight": dW2, "dense2.bias": red(dpv, chain_b, ov("db2")), "dense1.bias": red(o, chain_w, ov("colsum"))}


def bounds_six(x, rows_run, old=None):
    """Tolerances for exact_six's result.  rows_run: the DENSE row count B P -- both paths group and order their sums as the dense launches do.
    old (dict dW2 / db2 / colsum, optional): what the tail's three sums are accumulated into."""
    nr = H.n_reduce(H.box_bwd_blocks(rows_run))
    cw, cb = H.box_bwd_rpb(rows_run) + nr, 9 + nr
    if x["n"]:
        t = _tail_bounds(x["tail"], cw, cb, old)
    else:          # an empty list: every sum is an exact zero (an old value is kept as it is)
        z = lambda k: torch.full_like(x["grads"][k], TINY)
        t = {k: z(k) for k in ("dense2.weight", "dense2.bias", "dense1.bias")}
        t["du1"] = torch.zeros_like(x["du1"])
    Kp = (rows_run + 63) // 64 * 64
    gw = gamma2(n_acc(Kp) + 257)
    t["dense1.weight"] = gw * x["abs"]["dense1.weight"] + Kp * TINY
    t["dense0.weight"] = gw * x["abs"]["dense0.weight"] + Kp * TINY
    t["dense0.bias"] = gamma2(32 * (Kp // 64) + 1 + 257) * x["abs"]["dense0.bias"] + Kp * TINY
    return t


def make_case(rows, D, listed, seed=1, special=None):
    """Seeded CPU inputs of the kernels: dboxes f32 [rows, 4] that is zero outside `listed`, sig in (0, 1), bf16-exact hb1 / ub1 / hb0 / ub0 / feats
    [rows, D], w2 f32 [4, D], w1 bf16-exact [D, D].  special: {row: 4 values} overrides (NaN, -0.0, one component)."""
    g = torch.Generator(device="cpu").manual_seed(seed * 7919 + rows * 31 + D)
    rn = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t: t.to(torch.bfloat16).float()
    db = torch.zeros(rows, 4)
    if len(listed):
        db[torch.as_tensor(list(listed), dtype=torch.int64)] = rn(len(listed), 4)
    for r, v in (special or {}).items():
        db[r] = torch.tensor(v, dtype=torch.float32)
    return dict(dboxes=db, sig=torch.sigmoid(rn(rows, 4)), hb1=bf(rn(rows, D)), ub1=bf(1.5 * rn(rows, D)), hb0=bf(rn(rows, D)), ub0=bf(1.5 * rn(rows, D)),
                feats=bf(rn(rows, D)), w2=0.1 * rn(4, D), w1=bf(rn(D, D) / D ** 0.5))
