"""Float64 references, derived error bounds, input profiles and an f32 simulation for the fused attention kernels (checker side; device-agnostic:
every function works on whatever device its inputs live on).

Everything here works on ONE (image, head) chunk: q, k, v, dO are [T, 64] tensors whose values are bf16-exact.  Callers loop over chunks, so that
T = 3601 with 16 heads never holds more than a few [T, T] float64 matrices.

Two references
--------------
`exact_chunk`   softmax(Q K^T scale) V, its log-sum-exp in the log2 domain and dQ / dK / dV by the closed form, all in float64.
`emul_fwd_chunk`, `emul_bwd_chunk`
                the same in float64, but with the kernels' DETERMINISTIC rounding points (the ones tests/bf16_emulation.py::_AttnStore lists):
                  qs_fwd  forward scores come from bf16(c Q), c = f32(scale) * f32(log2 e)       attention_fwd.hip:170-179
                  ks_bwd  dK / dV kernel scores come from Q . bf16(c K)^T minus the given LSE    attention_bwd.hip:113-115
                  qs_bwd  dQ kernel scores come from bf16(c Q) . K^T minus the same LSE          attention_bwd.hip:297-299
                  D = rowsum(dO . O) on the STORED (bf16) O that is handed in                    attention_bwd.hip:59-80
                P and dS stay unrounded: their rounding is what the bounds below account for.  `rounding` names the points that are ON, so a
                violated bound can be localised by switching one off.  The backward takes the LSE and O it is given (the HIP forward's, in the GPU
                tests): the backward is judged as the kernel receives its inputs.
                The peeled forward's class-token row (attn_cls_row, attention_fwd_common.h:49-55) scales Q in f32 and does NOT round it to bf16:
                `emul_fwd_chunk(..., round_qs=False)` on that one row is its reference.

Bounds (elementwise, derived, no fitted constant)
-------------------------------------------------
u = 2^-8 is bf16's unit round-off (half an ulp, relative; the convention of test_gemm_model_row_counts), f = 2^-24 is f32's,
gamma(n) = n f / (1 - n f) bounds n chained f32 roundings.  Every bound is |kernel - emul| <= tol with tol built from:

 score error (all kernels).  A score is an f32 MFMA chain over 64 products (+ 2 slots for the offset / the -lse pair):
     ds = gamma(66) * (sum_d |a_d b_d| + |offset|)                                               attention_fwd.hip:249-253, attention_bwd.hip:211-219,371-380
   backward only: -lse enters as a (hi, lo) bf16 pair, hi = bf16(x), lo = bf16(x - hi): |x - hi| <= u |x| and |lo - (x - hi)| <= u^2 |x|, so
     ds += u^2 |lse| = 2^-16 |lse|                                                               attention_bwd.hip:40-43 (split_hi_lo_bf16)
   P~ = exp2(s~) (v_exp_f32, 1 ulp): relative error  eP = exp(ln2 ds) (1 + 2 f) - 1              attention_fwd.hip:274, attention_bwd.hip:226,386
 out.  N = sum_j bf16(p~_j) v_j in f32, L = sum_j p~_j in f32, out = bf16(N / L):
     |bf16(p~_j) - p_j| <= p_j ((1 + eP_j)(1 + u) - 1) =: w_j                                    attention_fwd.hip:324-326 (pack_bf2)
     E_N = sum_j w_j |v_j| + gamma(T) sum_j (p_j + w_j) |v_j|                                    attention_fwd.hip:336 (f32 MFMA accumulation over T keys)
     dL  = sum_j p_j eP_j + gamma(T) sum_j p_j (1 + eP_j)          (p normalised)                attention_fwd.hip:275,316,418
     E   = (E_N + |out| dL) / (1 - dL), then 2 more f32 roundings (1 / L, O * inv) and the bf16 store:
     tol_out = E' + u (|out| + E'),  E' = E + 2 f (|out| + E)                                    attention_fwd.hip:419,427 (pack_token_rows)
   To first order this is the issue's  u sum_j p_j |v_j| + u |out| + T 2^-24 sum_j p_j |v_j|.
 lse = M + log2(L~) (v_log_f32, 1 ulp of its result, then one f32 add):
     tol_lse = log2(1 + dL') + 2 f |log2 L~| + f |lse|,  dL' = dL / (1 - dL)                     attention_fwd.hip:434
   |log2 L~| = |lse - M|.  The offset M stays 0 (then |log2 L~| = |lse|) unless a tile's row sum leaves [2^-60, 2^88]
   (attention_fwd.hip:282), which needs a score beyond 88 - log2(64) = 82 or below -60; with an offset set, 2^-60 <= L~ <= T 2^88.  So
     |log2 L~| <= |lse| if max |score| of the chunk < 60, else 88 + log2 T.
   To first order: (T 2^-24 + sum p eP) / ln2 + 2^-23 |lse|, the issue's bound plus the score term.
 dvec = rowsum(dO . O) over the head's 64 features in f32: tol_dvec = gamma(64) sum_d |dO_d O_d|  attention_bwd.hip:72-79
 dP - D (f32 MFMA chain with the (hi, lo) pair of -D in front, D the kernel's own dvec):
     ddp = 2^-16 |D| + tol_dvec + gamma(66) (|D| + sum_d |dO_d v_d|)                             attention_bwd.hip:212-218,372-379
 dV = bf16(sum_q bf16(P~) dO):  W_P = P ((1 + eP)(1 + u) - 1)
     E = sum_q W_P |dO| + gamma(T) sum_q (P + W_P) |dO|;  tol_dV = E + u (|dV| + E)              attention_bwd.hip:229-237,249
 dS~ = bf16(P~ (dP - D)~), one f32 multiply then pack_bf2:
     W_S = P (1 + eP) (|dP - D| + ddp) (1 + f)(1 + u) - |dS|                                     attention_bwd.hip:227-231,391-394
   which to first order is |dS| (u + ln2 2^-16 |lse| + 2^-16 |D| / |dP - D| + ...), the issue's hi/lo term.
 dK = bf16(scale sum_q dS~ Q), dQ = bf16(scale sum_k dS~ K):
     E = scale (sum W_S |Q| + gamma(T) sum (|dS| + W_S) |Q|), E' = E + f (|dK| + E) (the scale multiply), tol = E' + u (|dK| + E')
                                                                                                 attention_bwd.hip:238,248,399,419
 flushed denormals.  v_exp_f32, the MFMAs and the bf16 conversions of these kernels do not keep denormals: a P~, dS~ or stored value below the
   smallest normal 2^-126 (f32 and bf16 share it) may become 0.  That is an ABSOLUTE error of 2^-126 per term, which the relative terms above cannot
   cover where a whole sum is that small (sink_mid120: every ordinary key holds P = 2^-120, so its dK is ~2^-124):
     tol_dV += (T max|dO| + 1) 2^-126;  tol_dK += (scale T max|Q| (1 + max|dP - D|) + 1) 2^-126  (P~ flushed inside dS~, dS~ itself, the store);
     tol_dQ likewise with max|K|.  Forward: the row sum L~ >= 2^-60 (attention_fwd.hip:282), so a flushed P~ is at most 2^-66 of the row:
     tol_out += T 2^-66 max|v| + 2^-126,  dL += T 2^-66.
"""
import math

import torch

U = 2.0 ** -8            # bf16 unit round-off
F = 2.0 ** -24           # f32 unit round-off
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
N_SCORE = 66             # contraction slots of a score chain that can hold a non-zero product: 64 features + the (hi, lo) / offset pair
VERDICT_LOG2 = 88.0      # attention_fwd_common.h: ATTN_VERDICT_LOG2
UNDERFLOW_LOG2 = 60.0    # attention_fwd.hip:282 (first tile: row sum < 2^-60)
TINY = 2.0 ** -126       # smallest normal f32 / bf16
L_MIN = 2.0 ** -UNDERFLOW_LOG2
ALL_ROUNDINGS = frozenset({"qs_fwd", "ks_bwd", "qs_bwd"})


def gamma(n):
    return n * F / (1.0 - n * F)


def bf16_round(x):
    """Round to bf16 (nearest even) and return in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def prescale(x, scale, rounded=True):
    """c x as the kernels form it: f32(x) * (f32(scale) * f32(log2 e)) in f32, then (rounded) one conversion to bf16 (scale_frag)."""
    c32 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    y = x.to(torch.float32) * c32.to(x.device)
    if rounded:
        y = y.to(torch.bfloat16)
    return y.to(torch.float64)


def _store(ref, E, f32_ops, floor):
    """Bound after `f32_ops` further f32 roundings and the bf16 store of a value that sits within E of `ref`; `floor` is the absolute term for
    flushed denormals (module docstring)."""
    E1 = E + f32_ops * F * (ref.abs() + E)
    return E1 + U * (ref.abs() + E1) + floor


def _rel_p(ds):
    return torch.exp(LN2 * ds) * (1.0 + 2.0 * F) - 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------------------------------------------------------
def exact_chunk(q, k, v, dO=None, scale=0.125):
    """float64 softmax attention of one chunk.  Returns a dict: out, lse (log2 domain) and, with dO, dq, dk, dv, dvec."""
    q, k, v = q.double(), k.double(), v.double()
    s = (q @ k.t()) * (scale * LOG2E)
    m = s.max(-1, keepdim=True).values
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    p = p / l
    r = {"out": p @ v, "lse": (m + torch.log2(l)).squeeze(-1)}
    if dO is not None:
        dO = dO.double()
        dvec = (dO * r["out"]).sum(-1, keepdim=True)
        ds = p * (dO @ v.t() - dvec)
        r.update(dv=p.t() @ dO, dk=scale * (ds.t() @ q), dq=scale * (ds @ k), dvec=dvec.squeeze(-1))
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------
# emulation of the deterministic rounding points, with bounds
# ---------------------------------------------------------------------------------------------------------------------------------------------
def emul_fwd_chunk(q, k, v, scale=0.125, round_qs=True, with_tol=True):
    """Forward with scores from bf16(c Q) (round_qs=False: from the f32 product c Q, the class-token row of the peeled tiling; or, with
    `scale * LOG2E` folded exactly, see emul_fwd_exact_scores).  Returns out, lse and (with_tol) tol_out, tol_lse; see the module docstring."""
    k, v = k.double(), v.double()
    qs = prescale(q, scale, rounded=round_qs)
    return _fwd_from_scaled(qs, k, v, with_tol)


def emul_fwd_exact_scores(q, k, v, scale=0.125):
    """`emul` with every rounding off: the scores are (q . k) * scale * log2(e) in float64.  Must equal exact_chunk."""
    return _fwd_from_scaled(q.double() * (scale * LOG2E), k.double(), v.double(), False)


def _fwd_from_scaled(qs, k, v, with_tol):
    T = k.shape[0]
    s = qs @ k.t()
    m = s.max(-1, keepdim=True).values
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    p = p / l
    lse = (m + torch.log2(l)).squeeze(-1)
    out = p @ v
    r = {"out": out, "lse": lse}
    if not with_tol:
        return r
    smax = float(s.abs().max())
    # the held offset M is the bf16 of a row maximum of an earlier tile: |M| <= (1 + u) max_j |s_j|
    ds = gamma(N_SCORE) * (qs.abs() @ k.abs().t() + (1.0 + U) * s.abs().max(-1, keepdim=True).values)
    eP = _rel_p(ds)
    w = p * ((1.0 + eP) * (1.0 + U) - 1.0)
    va = v.abs()
    E_N = w @ va + gamma(T) * ((p + w) @ va)
    dL = (p * eP).sum(-1, keepdim=True) + gamma(T) * (p * (1.0 + eP)).sum(-1, keepdim=True)
    E = (E_N + out.abs() * dL) / (1.0 - dL)
    r["tol_out"] = _store(out, E, 2, T * TINY / L_MIN * float(va.max()) + TINY)
    dLr = ((dL + T * TINY / L_MIN) / (1.0 - dL)).squeeze(-1)
    log_l = lse.abs() if smax < UNDERFLOW_LOG2 else torch.full_like(lse, VERDICT_LOG2 + math.log2(T))
    r["tol_lse"] = torch.log2(1.0 + dLr) + 2.0 * F * log_l + F * lse.abs()
    return r


def emul_bwd_chunk(q, k, v, dO, O, lse, scale=0.125, rounding=ALL_ROUNDINGS, with_tol=True):
    """Backward of one chunk as the kernels compute it from the LSE and the stored O they are given.  `rounding`: which of ks_bwd / qs_bwd are
    on (off: the float64 product c x, c = scale log2 e).  Returns dq, dk, dv, dvec and (with_tol) tol_dq, tol_dk, tol_dv, tol_dvec."""
    q, k, v, dO, O, lse = q.double(), k.double(), v.double(), dO.double(), O.double(), lse.double()
    T = q.shape[0]
    lse_c = lse.unsqueeze(-1)
    dvec = (dO * O).sum(-1, keepdim=True)
    r = {"dvec": dvec.squeeze(-1)}
    dpD = dO @ v.t() - dvec
    if with_tol:
        tol_dvec = gamma(64) * (dO * O).abs().sum(-1, keepdim=True)
        r["tol_dvec"] = tol_dvec.squeeze(-1)
        ddp = U * U * dvec.abs() + tol_dvec + gamma(N_SCORE) * (dvec.abs() + dO.abs() @ v.abs().t())

    def side(a, b):           # P and dS of one kernel: scores a . b^T - lse
        P = torch.exp2(a @ b.t() - lse_c)
        dS = P * dpD
        if not with_tol:
            return P, dS, None, None
        ds = U * U * lse_c.abs() + gamma(N_SCORE) * (lse_c.abs() + a.abs() @ b.abs().t())
        eP = _rel_p(ds)
        W_P = P * ((1.0 + eP) * (1.0 + U) - 1.0)
        W_S = P * (1.0 + eP) * (dpD.abs() + ddp) * ((1.0 + F) * (1.0 + U)) - dS.abs()
        return P, dS, W_P, W_S

    # dK / dV kernel
    ks = prescale(k, scale) if "ks_bwd" in rounding else k * (scale * LOG2E)
    P, dS, W_P, W_S = side(q, ks)
    r["dv"] = P.t() @ dO
    r["dk"] = scale * (dS.t() @ q)
    if with_tol:
        E = W_P.t() @ dO.abs() + gamma(T) * ((P + W_P).t() @ dO.abs())
        r["tol_dv"] = _store(r["dv"], E, 0, (T * float(dO.abs().max()) + 1.0) * TINY)
        E = scale * (W_S.t() @ q.abs() + gamma(T) * ((dS.abs() + W_S).t() @ q.abs()))
        r["tol_dk"] = _store(r["dk"], E, 1, (scale * T * float(q.abs().max()) * (1.0 + float(dpD.abs().max())) + 1.0) * TINY)
    del P, dS, W_P, W_S
    # dQ kernel
    qs = prescale(q, scale) if "qs_bwd" in rounding else q * (scale * LOG2E)
    P, dS, W_P, W_S = side(qs, k)
    r["dq"] = scale * (dS @ k)
    if with_tol:
        E = scale * (W_S @ k.abs() + gamma(T) * ((dS.abs() + W_S) @ k.abs()))
        r["tol_dq"] = _store(r["dq"], E, 1, (scale * T * float(k.abs().max()) * (1.0 + float(dpD.abs().max())) + 1.0) * TINY)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input profiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILES = ("randn", "peaked", "sink_first", "sink_last", "sink_mid80", "sink_mid120", "big_lse")
C = 0.125 * LOG2E          # dh = 64


def sink_mid_key(T):
    """The spiking key of sink_mid: key 250 (tile 3) as in test_attention_fwd_verdict_threshold_at_kernel_level; a later tile's key for short T."""
    return 250 if T > 314 else T - 30


def make_inputs(profile, B, H, T, seed):
    """Seeded, bf16-rounded inputs on the CPU: x [B, T, 3, H, 64] (q | k | v as the qkv rows hold them) and dO [B, T, H, 64], float32."""
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + B * 10007 + H * 101 + T)
    x = torch.randn(B, T, 3, H, 64, generator=g)
    dO = torch.randn(B, T, H, 64, generator=g)
    if profile == "randn":
        pass
    elif profile == "peaked":
        x[:, :, 0] *= 4.0
    elif profile in ("sink_first", "sink_last"):
        # sink key = 50 e (e a sign pattern per head); queries = randn + e / 4: the sink's log2 score is 72 (z + 2) with z ~ N(0, 1) -- in the hundreds
        # for most queries, which the sink then owns; every 8th query is CONTESTED instead: its component along e is set so that the sink weighs
        # about as much as all other keys together (log2 score ~ log2 T + 1), where a wrong weight of the sink shows in the output and in dS
        j = 0 if profile == "sink_first" else T - 1
        e = torch.sign(torch.randn(B, 1, H, 64, generator=g) + 1e-3)
        x[:, :, 0] += 0.25 * e
        x[:, j:j + 1, 1] = 50.0 * e
        cont = torch.arange(T) % 8 == 3
        qc = x[:, cont, 0]
        beta = (math.log2(T) + 1.0) / (C * 50.0 * 64.0)
        x[:, cont, 0] = qc - (qc * e).sum(-1, keepdim=True) * e / 64.0 + beta * e
    elif profile in ("sink_mid80", "sink_mid120"):
        # one key of a later tile `above` (log2) over the offset the wave holds (0: base scores ~ 1e-2), for every query of head 0
        above = float(profile[8:])
        x *= 0.05
        x[:, :, 0, 0, 0] = 8.0
        x[:, :, 1, 0, 0] = 0.0
        x[:, sink_mid_key(T), 1, 0, 0] = above / (8.0 * C)
    elif profile == "big_lse":
        # feature 0: queries +-8 (sign by row), every key 208: all scores of a row move by +-8 * 208 * c = +-300 (log2), so lse ~ +-300
        x[:, :, 0, :, 0] = torch.where(torch.arange(T) % 2 == 0, 8.0, -8.0).view(1, T, 1)
        x[:, :, 1, :, 0] = 208.0
    else:
        raise ValueError(profile)
    return bf16_round(x), bf16_round(dO)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation of the kernels' arithmetic (CPU tests: are the bounds wide enough for a correct kernel and tight enough for a wrong one?)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _split_hi_lo(x):
    hi = bf16_round(x)
    return hi + bf16_round(x - hi)


def simulate_fwd_f32(q, k, v, scale=0.125, defect=None):
    """The forward in f32 with bf16 P, bf16 output and f32 sums, against the bf16-exact row maximum.  `defect` breaks it on purpose:
    'leak7'    7 zero pad keys (and zero V rows) enter the softmax,
    'dup_last' the clamped duplicate of row T - 1 is not masked,
    'drop_tile' the keys 64..127 are left out of the PV product while the row sum keeps them (P not renormalised)."""
    q, k, v = q.float(), k.float(), v.float()
    if defect == "leak7":
        k = torch.cat([k, torch.zeros(7, 64)]); v = torch.cat([v, torch.zeros(7, 64)])
    elif defect == "dup_last":
        k = torch.cat([k, k[-1:]]); v = torch.cat([v, v[-1:]])
    qs = prescale(q, scale).float()
    s = qs @ k.t()
    m = bf16_round(s.max(-1, keepdim=True).values)
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    pb = bf16_round(p)
    if defect == "drop_tile":
        pb[:, 64:128] = 0.0
    out = bf16_round((pb @ v) * (1.0 / l))
    return out, (m + torch.log2(l)).squeeze(-1)


def simulate_bwd_f32(q, k, v, dO, O, lse, scale=0.125):
    """The backward in f32: -lse and -D as (hi, lo) bf16 pairs, bf16 P and dS, f32 sums, bf16 outputs.  Returns dq, dk, dv, dvec."""
    q, k, v, dO, O, lse = q.float(), k.float(), v.float(), dO.float(), O.float(), lse.float()
    dvec = (dO * O).sum(-1)
    nl = _split_hi_lo(-lse).unsqueeze(-1)
    nd = _split_hi_lo(-dvec).unsqueeze(-1)
    dp = dO @ v.t() + nd
    p1 = torch.exp2(q @ prescale(k, scale).float().t() + nl)
    dv = bf16_round(bf16_round(p1).t() @ dO)
    dk = bf16_round((bf16_round(p1 * dp).t() @ q) * scale)
    p2 = torch.exp2(prescale(q, scale).float() @ k.t() + nl)
    dq = bf16_round((bf16_round(p2 * dp) @ k) * scale)
    return dq, dk, dv, dvec


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol (NaN-safe: a NaN counts as infinite)."""
    err = (got.double() - ref).abs()
    r = err / tol
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())
