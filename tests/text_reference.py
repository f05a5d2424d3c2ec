"""Float64 references, derived error bounds, input profiles and an f32 simulation for the three kernels of csrc/text.hip: text_embed_kernel,
causal_attn_kernel and text_pool_kernel (the entries owl_text_embed, owl_causal_attention_small, owl_text_pool_project).  Checker side;
device-agnostic: every function works on whatever device its inputs live on, and nothing here imports the package's Python ops.

Reference (float64 on the kernel's exact inputs: bf16 values upcast, f32 values, eps as the f32 the launcher receives)
---------
`exact_embed(ids [N, S], tok [vocab, W], pos [>= S, W])`   tok[clamp(id, 0, vocab - 1)] + pos[m % S] for row m = n S + t       text.hip:14-19
    `embed_f32` is the same with ONE torch f32 add (not taken from the code under test): the kernel's result is asserted bit for bit against it.
`exact_attention(qkv [N S, 3 W], N, S, heads, scale)`   per (sequence n, head h): s_ij = scale q_i . k_j, softmax over j <= i, out_i = sum_j p_ij v_j;
    q | k | v of token m, head h are the columns h 64 + d, W + h 64 + d, 2 W + h 64 + d of row m (W = 64 heads)                   text.hip:28-33,39
`exact_pool(x [N S, W], ids, gamma, beta, wproj [Pdim, W], eps)`   eos = FIRST position of the row's maximal id (text.hip:70-74), LayerNorm of that row
    (population variance, eps inside the root, text.hip:82-90), o = wproj y (no bias, text.hip:92-98), out = o / |o|_2 (text.hip:100-107).

What hipcc emits for gfx950 (read from `hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only text.hip` with the flags of csrc/build.sh; text.hip has
no -ffp-contract override, so the compiler contracts where it likes) -- the simulation follows THIS, the bounds hold for either form of every chain:
 score (text.hip:44)      v_fma_f32 s, q0, k0, 0; 51 v_fmac_f32 (d = 1..51); d = 52..63 as v_pk_mul_f32 (a rounded product) + v_add_f32, in order of d.
 __expf (text.hip:46)     v_sub_f32; v_mul_f32 by 0x3fb8aa3b (f32(log2 e)); v_exp_f32 -- no range scaling around it, so a result below 2^-126 is flushed to 0.
 l (text.hip:47)          v_fmac_f32 p += l corr: one rounding.
 acc (text.hip:49)        v_pk_mul_f32 p v (rounded), then v_pk_fma_f32 corr acc + (p v): two roundings for the new term, one for the old sum.
 1 / l (text.hip:52)      v_div_scale / v_rcp / fma refinement / v_div_fmas / v_div_fixup: the correctly rounded division; acc inv is v_pk_mul_f32, the store
                          v_cvt_pk_bf16_f32 (RNE).  The same division sequence forms sum / W twice (text.hip:82,89) and o / nrm (text.hip:107).
 pool sums (text.hip:78)  v_add_f32 per column; variance: v_sub_f32 then v_fmac_f32 v += d d (the square is NOT rounded); wave_sum: 6 ds_bpermute + v_add_f32;
                          the four partials ((r0 + r1) + r2) + r3 by v_add_f32.
 rstd (text.hip:89)       v_add_f32 eps, v_rsq_f32 (behind a scaling of arguments below 2^-126 that var + eps >= eps never takes).
 y (text.hip:90)          v_sub / v_mul rstd (row - mean) / v_fma gamma t + beta  (pk forms in the unrolled body): three roundings.
 projection (text.hip:95) v_fmac_f32 a += y w, one wave per output, columns strided by 64; six butterfly levels.
 norm (text.hip:101-106)  v_fmac_f32 q += o o; butterfly; three adds; v_sqrt_f32 with the one-ulp fix-up sequence (correctly rounded).
Kernels run with f32 denormals kept (.amdhsa_float_denorm_mode_32 3); only v_exp_f32 / v_rsq_f32 / v_sqrt_f32 / v_rcp_f32 results can be flushed.

Bounds (elementwise |kernel - exact| <= tol, derived, no fitted constant)
------
u = 2^-8, f = 2^-24, T = 2^-126, gamma(n) = n f / (1 - n f): gemm_reference.py:18-20, imported.  A division, v_sqrt and 1 / l are budgeted ONE ULP = 2 f each although
the sequences above are the correctly rounded ones (f): the bound does not rest on that reading.  ASSUMPTION 1 of layernorm_reference.py (v_rsq_f32 within
2 ulp = 4 f) is taken over with its constant.
 embed.  One f32 add (text.hip:19):  tol = f |tok + pos| + T.  (The GPU test asserts the bits of `embed_f32`, which is stronger.)
 attention, row i of one (sequence, head); s_j, p_j (normalised), out exact; m = max_j s_j:
   score (text.hip:39,44).  q_d scale is one rounding, the chain over d at most 64 more for the first product (fewer for the later ones, and fewer again
     where a product is fused):        ds_j = gamma(65) scale sum_d |q_d k_d| + T         (`N_SCORE` = 65)
   __expf of an argument a <= 0 (text.hip:46).  a~ = fl(x - nm) (f), t = fl(a~ c), c = f32(log2 e) within f of log2 e (f, f): t = a log2 e (1 + th), |th| <= gamma(3),
     so 2^t = e^a e^(a th): the argument-scaling term, PROPORTIONAL to |a| = |s - nm|; v_exp_f32 is 1 ulp = 2 f:
                                       rexp(a) = exp(gamma(3) |a|) (1 + 2 f) - 1.     a = 0 gives exactly 1 (corr of a step that does not raise the maximum, p of the one that does).
   the recurrence (text.hip:41-51).  After key i the weight of key j is  p~_j prod_{t > j} corr~_t;  exactly, exp(s~_j - nm_j) prod exp(mx_{t-1} - nm_t) = exp(s~_j - m~)
     (the arguments telescope and all have one sign), so the argument-scaling terms ADD UP to gamma(3) (m~ - s~_j) however many steps raise the maximum -- the one bound
     of the corr chain -- and each of the n_j = i - j later steps adds one v_exp ulp and one fma rounding; the product p v adds one rounding (acc only):
       a_j  = (m - s_j) + ds_j + max_k ds_k                  (m~ - s~_j in terms of exact scores)
       eN_j = exp(ds_j) exp(gamma(3) a_j) (1 + 2 f)^(n_j + 1) (1 + f)^(n_j + 2) - 1       relative error of key j's term of acc   (text.hip:49)
       eL_j = exp(ds_j) exp(gamma(3) a_j) (1 + 2 f)^(n_j + 1) (1 + f)^(n_j + 1) - 1       ... of l                                  (text.hip:47)
     (exp(ds_j): the score's own error; the common factor exp(m - m~) cancels between acc and l.)
       E_N = sum_j p_j eN_j |v_j|,  dL = sum_j p_j eL_j,  E = (E_N + |out| dL) / (1 - dL)
   output (text.hip:52,55).  inv = 1 / l (2 f), acc inv (f), bf16 store (u):  E' = E + 3 f (|out| + E),  tol = E' + u (|out| + E') + floor
   flushed denormals.  l~ >= 1 (the key that holds the maximum enters with p = 1 and later corr = 1), so a weight whose p or corr falls below T and is flushed loses
     at most T (1 + eN) of a row sum >= 1; products below T keep their denormals but round absolutely (T f each, below T):
       floor = 2 (i + 1) T (max |v| + |out|) + T
 pool (one row v [W] of f32, exact inputs), nv = ceil(W / 256):
   chains.  n_stat(W) = ceil(W / 256) + 6 + 3   a thread's strided adds (text.hip:78,85), six butterfly levels (common.h:142-146), the four wave partials in order
            n_proj(W) = ceil(W / 64) + 6        (text.hip:95-96)          n_norm(P) = ceil(P / 256) + 6 + 3   (text.hip:101-106)
            -- the helpers the simulation's own count is held to (test_text_reference.py::test_chain_lengths_are_the_ones_the_simulation_performs).
   mean~ = fl(S~ / W), the division 2 f:            E_mean = gamma(n_stat + 2) sum |v| / W + T                                             text.hip:78-82
   d~ = fl(v - mean~):                               E_d = E_mean + E_dI,  E_dI = f (|d| + E_mean) its own rounding                          text.hip:85
   variance, two passes: sum (d_i - dm)^2 - sum d_i^2 = W dm^2 because sum d_i = 0 (layernorm_reference.py:30-35); the rounding of d~ costs r2 q per square,
     q = (|d| + E_mean)^2, r2 = (1 + f)^2 - 1; the squares are fused:
       E_var = (sum (E_mean^2 + r2 q) + gamma(n_stat + 2) sum (1 + r2) q) / W + T                                                            text.hip:85-89
       ve~ = fl(var~ + eps): E_ve = E_var + f (ve + E_var), rho = E_ve / ve;  r_rstd = (1 + 4 f) (1 - rho)^-1/2 - 1,  E_rstd = rstd r_rstd   text.hip:89
   y = fma(g, fl(rstd~ d~), b):  E_t = mul(d, E_d, rstd, E_rstd) + f (.),  E_y = |g| E_t + f (|y| + |g| E_t) + T                              text.hip:90
   o_p = sum_c y_c w_pc by fma.  The error of the mean, dm, moves EVERY y_c of the row by -dm rstd g_c: that part of E_y, |g_c| rstd E_mean, is one number times a known
     vector and enters o_p as dm rstd sum_c g_c w_pc -- bounded with the SIGNED sum, not with sum_c |g_c w_pc| (sqrt(W) times more at a large mean, where a
     one-pass variance would hide under it);  E_yB = E_y - |g| rstd E_mean is the rest:
       E_o = rstd E_mean |sum_c g_c w_pc| + sum_c E_yB |w| + gamma(n_proj) sum_c (|y| + E_y) |w| + T                                         text.hip:92-98
   nrm~ = sqrt~(q~), q~ the fma chain over o~^2 (all terms >= 0: relative gamma(n_norm)), the root 2 f:
       nrm~ = |o~|_2 (1 + r),  |r| <= r_n = (1 + gamma(n_norm))^1/2 (1 + 2 f) - 1;  | |o~|_2 - |o|_2 | <= |E_o|_2                             text.hip:100-106
       E_nrm = |E_o|_2 + r_n (|o|_2 + |E_o|_2)
   out = fl(o~ / nrm~), the division 2 f:  E = (E_o + |out| E_nrm) / (nrm - E_nrm),  tol = E + 2 f (|out| + E) + T                            text.hip:107
   norm of an output row: |out~|_2 = |o~|_2 / nrm~ up to the divisions' 2 f, whatever E_o is:   | |out~|_2 - 1 | <= (1 + 2 f) / (1 - r_n) - 1 =: `tol_norm`.
   A projected row of exact zeros is 0 / 0 in HF too and is the one input the profiles exclude.

Profiles -- what each is meant to reach; test_text_reference.py asserts that it reaches it
--------
 attention (`make_attn_inputs`, q / k / v bf16-exact; e is a +-1 pattern per (sequence, head), q_i = (1 + u_i / 4) e so that q_i . e scale = 8 (1 + u_i / 4)):
   randn       the baseline.                          ascending   k_j = j e + noise: every later key beats the running maximum by about 8: corr < 1 at every step.
   descending  k_j = (S - 1 - j) e + noise: key 0 holds the maximum, corr == 1 at every later step.
   sink_first  key 0 = 7.5 e, about 60 above randn keys.
   late_spike  key S - 2 = 10 e, about 80 above the rest: rows >= S - 2 rescale a large acc to almost zero (exp(-80) ~ 2^-115, still a normal f32).
   equal       every key the same vector: all scores of a row identical.
 pool rows (`make_pool_inputs`): randn (2 randn + 0.3); offset (mean +-100, spread 1: a one-pass variance loses it); flat (a constant row: y = beta up to eps);
   outlier (unit rows with columns 0, W - 1 and up to two more at +-(64 ... 256)).  EOS placements `EOS_KINDS`: first / last position, a tie of two maximal ids, all ids equal.

`emulate_*` simulate the kernels' arithmetic in f32 in the order listed above and take `hooks` that plant errors; with dtype=float64 every rounding is off
and they must equal `exact_*`.  They serve the CPU test only and are NEVER a reference on the GPU.
"""
import math

import torch

from tests.gemm_reference import F, TINY, U, _fma32, bf16_round, bits, check, gamma as gam, ratios, untouched  # noqa: F401
from tests.layernorm_reference import RSQRT_ULPS, _mul, _wave_sum, eps32

DH = 64
SCALE = 0.125
N_SCORE = DH + 1         # the scale multiply + 64 chained operations
N_ARG = 3                # fl(x - nm), f32(log2 e), fl(a c)
DIV = 2.0 * F            # budget of a division, v_sqrt and 1 / l (module docstring)
WAVES = 4
LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))        # 0x3fb8aa3b
N_FUSED = 52             # products d < 52 of a score are fused, d >= 52 rounded and added


def n_thread(W):
    return (W + 255) // 256


def n_stat(W):
    return n_thread(W) + 6 + (WAVES - 1)


def n_proj(W):
    return (W + 63) // 64 + 6


def n_norm(P):
    return n_thread(P) + 6 + (WAVES - 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# embed
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _embed_rows(ids, S, vocab, hooks=()):
    idf = ids.reshape(-1)
    m = torch.arange(idf.numel(), device=idf.device)
    t = torch.div(m, S, rounding_mode="floor") if "pos_div" in hooks else m % S
    return idf.clamp(0, vocab - 1), t, (idf < 0) | (idf >= vocab)


def exact_embed(ids, tok, pos):
    row, t, _ = _embed_rows(ids, ids.shape[1], tok.shape[0])
    return tok.double()[row] + pos.double()[t]


def embed_f32(ids, tok, pos):
    row, t, _ = _embed_rows(ids, ids.shape[1], tok.shape[0])
    return tok.float()[row] + pos.float()[t]


def bounds_embed(ref):
    return F * ref.abs() + TINY


def emulate_embed(ids, tok, pos, hooks=()):
    """hooks: "pos_div" (position m / S; rows past the table read NaN), "no_clamp" (an id outside [0, vocab) reads NaN, the stand-in for whatever lies
    outside the table)."""
    row, t, outside = _embed_rows(ids, ids.shape[1], tok.shape[0], hooks)
    p = torch.full((max(int(t.max()) + 1, pos.shape[0]), pos.shape[1]), float("nan"))
    p[:pos.shape[0]] = pos.float()
    x = tok.float()[row] + p[t]
    if "no_clamp" in hooks:
        x[outside] = float("nan")
    return x


# ---------------------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------------------
def split_qkv(qkv, N, S, heads):
    """qkv [>= N S, 3 W] -> q, k, v [N, heads, S, 64] (views of the first N S rows)."""
    x = qkv[:N * S].reshape(N, S, 3, heads, DH)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def merge_heads(o):
    """[N, heads, S, 64] -> [N S, W]"""
    N, H, S, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(N * S, H * DH)


def _causal(S, device):
    i = torch.arange(S, device=device)
    return i[None, :] <= i[:, None]                   # [i, j]


def exact_attention(qkv, N, S, heads, scale=SCALE):
    """-> dict out [N S, W] float64 and the intermediates the bounds need (q, k, v, s, p [N, heads, S, S], keep)."""
    q, k, v = (t.double() for t in split_qkv(qkv, N, S, heads))
    s = (q @ k.transpose(-1, -2)) * float(torch.tensor(scale, dtype=torch.float32))
    keep = _causal(S, qkv.device)
    sm = s.masked_fill(~keep, float("-inf"))
    m = sm.max(-1, keepdim=True).values
    p = torch.exp(sm - m)
    p = p / p.sum(-1, keepdim=True)
    o = p @ v
    return {"out": merge_heads(o), "o": o, "q": q, "k": k, "v": v, "s": s, "m": m, "p": p, "keep": keep, "scale": abs(float(scale))}


def bounds_attention(r):
    """-> tol [N S, W] (module docstring)."""
    q, k, v, s, m, p, keep, o = r["q"], r["k"], r["v"], r["s"], r["m"], r["p"], r["keep"], r["o"]
    S = s.shape[-1]
    ds = gam(N_SCORE) * r["scale"] * (q.abs() @ k.abs().transpose(-1, -2)) + TINY
    ds = ds.masked_fill(~keep, 0.0)
    a = (m - s).masked_fill(~keep, 0.0) + ds + ds.max(-1, keepdim=True).values
    idx = torch.arange(S, device=s.device)
    nj = (idx[:, None] - idx[None, :]).clamp(min=0).double()                 # [i, j]: steps after key j
    common = torch.exp(ds + gam(N_ARG) * a) * (1.0 + 2.0 * F) ** (nj + 1.0)
    eN = common * (1.0 + F) ** (nj + 2.0) - 1.0
    eL = common * (1.0 + F) ** (nj + 1.0) - 1.0
    E_N = (p * eN) @ v.abs()
    dL = (p * eL).sum(-1, keepdim=True)
    E = (E_N + o.abs() * dL) / (1.0 - dL)
    E1 = E + 3.0 * F * (o.abs() + E)
    vmax = v.abs().amax((-1, -2), keepdim=True)
    floor = 2.0 * (idx + 1.0).double()[:, None] * TINY * (vmax + o.abs()) + TINY
    return merge_heads(E1 + U * (o.abs() + E1) + floor)


def _fma(a, b, c):
    """fma in the dtype of the simulation: one rounding in f32, plain arithmetic in float64 (the no-rounding run)."""
    return _fma32(a, b, c) if a.dtype == torch.float32 else a * b + c


def _expf(x):
    """__expf as compiled: v_exp_f32(fl(x f32(log2 e))), results below 2^-126 flushed; float64: exp."""
    if x.dtype == torch.float64:
        return torch.exp(x)
    r = torch.exp2(x * torch.tensor(LOG2E32, dtype=torch.float32))
    return torch.where(r < TINY, torch.zeros_like(r), r)


def emulate_attention(qkv, N, S, heads, scale=SCALE, hooks=(), dtype=torch.float32, plant_ulp=None):
    """causal_attn_kernel on the CPU -> out [N S, W] (bf16 values in float32; float64 and unrounded for dtype=float64).
    hooks: "mask_lt" (j < i), "mask_le_ip1" (j <= i + 1, within the sequence), "no_scale", "scale_twice", "no_corr_acc", "no_corr_l", "v_from_k",
    "no_head_offset" (every head reads head 0's q, k, v).  plant_ulp = (row, col): one bf16 ulp is added to that output."""
    q, k, v = (t.to(dtype).contiguous() for t in split_qkv(qkv.cpu(), N, S, heads))
    if "v_from_k" in hooks:
        v = k
    if "no_head_offset" in hooks:
        q, k, v = (t[:, :1].expand(-1, heads, -1, -1) for t in (q, k, v))
    sc = torch.tensor(scale, dtype=torch.float32).to(dtype)
    qs = q if "no_scale" in hooks else q * sc
    if "scale_twice" in hooks:
        qs = qs * sc
    s = torch.zeros(N, heads, S, S, dtype=dtype)
    for d in range(DH):
        a, b = qs[..., :, None, d], k[..., None, :, d]
        s = _fma(a.expand_as(s), b.expand_as(s), s) if d < N_FUSED else s + a * b
    i = torch.arange(S)
    mx = torch.full((N, heads, S), float("-inf"), dtype=dtype)
    l = torch.zeros(N, heads, S, dtype=dtype)
    acc = torch.zeros(N, heads, S, DH, dtype=dtype)
    one = torch.ones((), dtype=dtype)
    for j in range(S):
        if "mask_lt" in hooks:
            act = j < i
        elif "mask_le_ip1" in hooks:
            act = j <= i + 1
        else:
            act = j <= i
        sj = s[..., j]
        nm = torch.maximum(mx, sj)
        corr, p = _expf(mx - nm), _expf(sj - nm)
        l2 = _fma(l, one if "no_corr_l" in hooks else corr, p)
        ca = (one if "no_corr_acc" in hooks else corr)[..., None].expand_as(acc)
        acc2 = _fma(ca, acc, p[..., None] * v[..., j:j + 1, :])
        mx, l, acc = torch.where(act, nm, mx), torch.where(act, l2, l), torch.where(act[:, None], acc2, acc)
    out = merge_heads(acc * (one / l)[..., None])
    if dtype == torch.float64:
        return out
    out = bf16_round(out)
    if plant_ulp is not None:
        b = out.to(torch.bfloat16).view(torch.int16)
        b[plant_ulp] += 1                          # next bf16 away from zero
        out = b.view(torch.bfloat16).float()
    return out


ATTN_PROFILES = ("randn", "ascending", "descending", "sink_first", "late_spike", "equal")
ATTN_SHAPES = ((1, 1, 1), (2, 2, 1), (3, 16, 8), (1, 17, 12), (2, 63, 2), (2, 64, 3))       # (N, S, heads)


def make_attn_inputs(profile, N, S, heads, seed):
    """Seeded bf16-exact qkv [N S, 3 W] float32 on the CPU (module docstring)."""
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + N * 10007 + S * 101 + heads)
    x = torch.randn(N, S, 3, heads, DH, generator=g)
    e = torch.sign(torch.randn(N, 1, heads, DH, generator=g) + 1e-3)
    u = torch.rand(N, S, heads, 1, generator=g)
    noise = 0.25 * torch.randn(N, S, heads, DH, generator=g)
    pos = torch.arange(S, dtype=torch.float32).view(1, S, 1, 1)
    if profile == "randn":
        pass
    elif profile in ("ascending", "descending"):
        x[:, :, 0] = (1.0 + 0.25 * u) * e
        x[:, :, 1] = (pos if profile == "ascending" else (S - 1) - pos) * e + noise
    elif profile == "sink_first":
        x[:, :, 0] = e + 0.5 * x[:, :, 0]
        x[:, 0, 1] = 7.5 * e[:, 0]
    elif profile == "late_spike":
        x[:, :, 0] = e + 0.5 * x[:, :, 0]
        if S >= 2:
            x[:, S - 2, 1] = 10.0 * e[:, 0]
    elif profile == "equal":
        x[:, :, 1] = x[:, :1, 1]
    else:
        raise ValueError(profile)
    return bf16_round(x).reshape(N * S, 3 * heads * DH)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# pool
# ---------------------------------------------------------------------------------------------------------------------------------------------
def first_max(ids):
    """first position of the row's maximal id (written without argmax: no reliance on its tie rule)."""
    S = ids.shape[1]
    pos = torch.arange(S, device=ids.device).expand_as(ids)
    return torch.where(ids == ids.max(1, keepdim=True).values, pos, torch.full_like(pos, S)).min(1).values


def last_max(ids):
    S = ids.shape[1]
    pos = torch.arange(S, device=ids.device).expand_as(ids)
    return torch.where(ids == ids.max(1, keepdim=True).values, pos, torch.full_like(pos, -1)).max(1).values


def exact_pool(x, ids, gamma, beta, wproj, eps):
    N, S = ids.shape
    eos = first_max(ids)
    v = x[torch.arange(N, device=x.device) * S + eos].double()
    e = eps32(eps)
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + e)
    g, b, w = gamma.double(), beta.double(), wproj.double()
    y = d * rstd * g + b
    o = y @ w.t()
    nrm = torch.sqrt((o * o).sum(-1, keepdim=True))
    return {"out": o / nrm, "eos": eos, "v": v, "mean": mean, "d": d, "var": var, "rstd": rstd, "y": y, "o": o, "nrm": nrm, "eps": e, "g": g, "w": w}


def bounds_pool(r):
    """-> {"out": tol [N, Pdim], "norm": tol of | |out|_2 - 1 |} (module docstring)."""
    v, d, var, rstd, y, o, nrm, g, w = r["v"], r["d"], r["var"], r["rstd"], r["y"], r["o"], r["nrm"], r["g"], r["w"]
    W, P = v.shape[-1], o.shape[-1]
    ns = n_stat(W)
    E_mean = gam(ns + 2) * v.abs().sum(-1, keepdim=True) / W + TINY
    E_dI = F * (d.abs() + E_mean)                                # the part of d~'s error that is NOT the row's common shift dm
    r2 = (1.0 + F) ** 2 - 1.0
    q = (d.abs() + E_mean) ** 2
    E_var = ((E_mean * E_mean + r2 * q).sum(-1, keepdim=True) + gam(ns + 2) * ((1.0 + r2) * q).sum(-1, keepdim=True)) / W + TINY
    ve = var + r["eps"]
    E_ve = E_var + F * (ve + E_var)
    rho = E_ve / ve
    E_rstd = rstd * ((1.0 + RSQRT_ULPS * 2.0 * F) / torch.sqrt(1.0 - rho) - 1.0)
    t = d * rstd
    E_t = _mul(d, E_mean + E_dI, rstd, E_rstd)
    E_t = E_t + F * (t.abs() + E_t)
    shift = rstd * E_mean                                         # |g_c| shift is the common part of E_y: it enters o_p as dm rstd sum_c g_c w_pc
    E_y = g.abs() * E_t + F * (y.abs() + g.abs() * E_t) + TINY
    E_yB = E_y - g.abs() * shift
    E_o = shift * (g @ w.t()).abs() + E_yB @ w.abs().t() + gam(n_proj(W)) * ((y.abs() + E_y) @ w.abs().t()) + TINY
    r_n = math.sqrt(1.0 + gam(n_norm(P))) * (1.0 + DIV) - 1.0
    E_o2 = torch.sqrt((E_o * E_o).sum(-1, keepdim=True))
    E_nrm = E_o2 + r_n * (nrm + E_o2)
    out = r["out"]
    E = (E_o + out.abs() * E_nrm) / (nrm - E_nrm)
    return {"out": E + DIV * (out.abs() + E) + TINY, "norm": (1.0 + DIV) / (1.0 - r_n) - 1.0}


def _strided_sum(vals, lanes, fused_sq=False, counts=None, key=None, drop_wave3=False):
    """sum over the last axis of vals [R, n] as a workgroup / a wave does it: thread t adds columns t, t + lanes, ... in order (with fused_sq the term is
    d d by fma), six butterfly levels per wave, then (lanes = 256) the four wave partials in order.  -> [R, 1]"""
    R, n = vals.shape
    per = (n + lanes - 1) // lanes
    buf = torch.zeros(R, per * lanes, dtype=vals.dtype)
    buf[:, :n] = vals
    buf = buf.reshape(R, per, lanes)
    s = torch.zeros(R, lanes, dtype=vals.dtype)
    for i in range(per):                               # (a thread without a column at round i adds nothing: + 0 and fma(0, 0, s) are exact)
        s = _fma(buf[:, i], buf[:, i], s) if fused_sq else s + buf[:, i]
    cnt = [per]
    w = _wave_sum(s.reshape(R * (lanes // 64), 64), cnt)[:, 0].reshape(R, lanes // 64)
    if lanes == 256:
        tot = (w[:, 0] + w[:, 1]) + w[:, 2]
        tot = tot if drop_wave3 else tot + w[:, 3]
        cnt[0] += WAVES - 1
    else:
        tot = w[:, 0]
    if counts is not None:
        counts[key] = cnt[0]
    return tot[:, None]


def emulate_pool(x, ids, gamma, beta, wproj, eps, hooks=(), dtype=torch.float32, counts=None):
    """text_pool_kernel on the CPU -> out [N, Pdim].  hooks: "last_eos", "var_wm1" (variance over W - 1), "no_eps", "wproj_T" (wproj indexed [c][p]),
    "no_norm", "drop_wave3" (the fourth wave's partial left out of the mean), "one_pass" (E[x^2] - mean^2)."""
    N, S = ids.shape
    eos = last_max(ids) if "last_eos" in hooks else first_max(ids)
    v = x.cpu()[torch.arange(N) * S + eos.cpu()].to(dtype)
    W = v.shape[1]
    Wf = torch.tensor(float(W), dtype=dtype)
    e = torch.zeros((), dtype=dtype) if "no_eps" in hooks else torch.tensor(eps, dtype=torch.float32).to(dtype)
    g, b, w = gamma.cpu().to(dtype), beta.cpu().to(dtype), wproj.cpu().to(dtype)
    if "wproj_T" in hooks:                         # element (p, c) read at c Pdim + p of the buffer: the transpose when Pdim == W
        w = w.reshape(W, w.shape[0]).t().contiguous()
    mean = _strided_sum(v, 256, counts=counts, key="n_stat", drop_wave3="drop_wave3" in hooks) / Wf
    if "one_pass" in hooks:
        var = _strided_sum(v, 256, fused_sq=True) / Wf - mean * mean
    else:
        var = _strided_sum(v - mean, 256, fused_sq=True) / (Wf - 1.0 if "var_wm1" in hooks else Wf)
    rstd = torch.rsqrt(var + e)
    y = _fma(g.expand_as(v), rstd * (v - mean), b.expand_as(v))
    P = w.shape[0]
    o = torch.zeros(N, P, dtype=dtype)
    per = (W + 63) // 64
    yb = torch.zeros(N, per * 64, dtype=dtype)
    yb[:, :W] = y
    wb = torch.zeros(P, per * 64, dtype=dtype)
    wb[:, :W] = w
    a = torch.zeros(N, P, 64, dtype=dtype)
    for i in range(per):
        a = _fma(yb[:, None, i * 64:(i + 1) * 64].expand_as(a), wb[None, :, i * 64:(i + 1) * 64].expand_as(a), a)
    cnt = [per]
    o = _wave_sum(a.reshape(N * P, 64), cnt)[:, 0].reshape(N, P)
    if counts is not None:
        counts["n_proj"] = cnt[0]
    if "no_norm" in hooks:
        return o
    nrm = torch.sqrt(_strided_sum(o, 256, fused_sq=True, counts=counts, key="n_norm"))
    return o / nrm


POOL_PROFILES = ("randn", "offset", "flat", "outlier")
POOL_SHAPES = ((1, 1, 64, 64), (5, 16, 64, 40), (2, 7, 320, 7), (3, 16, 512, 512), (2, 16, 768, 768))     # (N, S, W, Pdim)
EOS_KINDS = ("first", "last", "tie", "all_equal")
VOCAB = 97
EPS = 1e-5


def make_ids(kind, N, S, seed, vocab=VOCAB):
    """[N, S] int64: ordinary ids in [1, vocab - 2] with the maximal id vocab - 1 placed by `kind`; ("tie": two of them, the second last in the row)."""
    g = torch.Generator(device="cpu").manual_seed(seed * 7919 + N * 131 + S)
    ids = torch.randint(1, vocab - 1, (N, S), generator=g)
    if kind == "first":
        ids[:, 0] = vocab - 1
    elif kind == "last":
        ids[:, S - 1] = vocab - 1
    elif kind == "tie":
        ids[:, S // 2] = vocab - 1
        ids[:, S - 1] = vocab - 1
    elif kind == "all_equal":
        ids[:] = 5
    else:
        raise ValueError(kind)
    return ids


def make_pool_inputs(profile, N, S, W, Pdim, seed):
    """Seeded f32 inputs on the CPU: x [N S, W], gamma, beta [W], wproj [Pdim, W]; every row of x is different, so that pooling another row shows."""
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + N * 10007 + S * 1009 + W * 101 + Pdim)
    R = N * S
    n = torch.randn(R, W, generator=g)
    sign = torch.where(torch.rand(R, 1, generator=g) < 0.5, -1.0, 1.0)
    if profile == "randn":
        x = 2.0 * n + 0.3
    elif profile == "offset":
        x = n + 100.0 * sign
    elif profile == "flat":
        x = ((0.5 + torch.rand(R, 1, generator=g)) * sign).expand(R, W).clone()
    elif profile == "outlier":
        x = n.clone()
        cols = [0, W - 1] + (torch.randperm(W - 2, generator=g)[:2] + 1).tolist()
        for c in cols:
            x[:, c] = (64.0 + 192.0 * torch.rand(R, generator=g)) * torch.where(torch.rand(R, generator=g) < 0.5, -1.0, 1.0)
    else:
        raise ValueError(profile)
    return {"x": x.float().contiguous(), "gamma": (1.0 + 0.1 * torch.randn(W, generator=g)).float(), "beta": (0.5 * torch.randn(W, generator=g)).float(),
            "wproj": (torch.randn(Pdim, W, generator=g) / math.sqrt(W)).float().contiguous()}


EMBED_SHAPES = ((1, 1, 64, 97), (3, 5, 128, 97), (5, 3, 320, 97), (2, 16, 512, 1000))        # (N, S, W, vocab)


def make_embed_inputs(N, S, W, vocab, seed, max_pos=16):
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + N * 10007 + S * 1009 + W)
    return {"ids": torch.randint(0, vocab, (N, S), generator=g), "tok": torch.randn(vocab, W, generator=g), "pos": torch.randn(max_pos, W, generator=g)}
