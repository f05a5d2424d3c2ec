"""Float64 references, derived error bounds, input profiles and an f32 simulation for the weight-gradient path: the TN split-K GEMM of
csrc/gemm_tn.hip (gemm_tn_slab_kernel, gemm_tn_pp_kernel and the bias fold of the latter), owl_slab_reduce (gemm.hip) and the column-sum kernels of
csrc/backward.hip (colsum_bf16_kernel, colsum_f32_kernel, transpose_colsum_kernel, each followed by partials_reduce_kernel).  Checker side;
device-agnostic: every function works on whatever device its inputs live on.  The conventions (u, f, gamma, gamma2, n_acc, T, ASSUMPTION 1) are those of
tests/gemm_reference.py and are imported from it, not restated.

Split rule (owl_gemm_tn_slab_bf16, gemm_tn.hip:405-408; owl_gemm_tn_slab_workspace_bytes, gemm_tn.hip:388-391)
--------------------------------------------------------------------------------------------------------------
    nk = ceil(M / 64),  splits = min(splits, nk),  per = ceil(nk / splits),  nsplit = ceil(nk / per)
Split s covers the K-tiles [per s, min(nk, per (s + 1))), that is the tokens Ts = [64 per s, min(M, 64 per (s + 1))) (`split_rule`).

Reference
---------
`exact_tn(dy, x, rows, n_out, n_in, splits, old_w, old_b)` in float64 on bf16-exact operands dy [>= rows, >= n_out], x [>= rows, >= n_in]:
    slab[s] = dy[Ts]^T x[Ts]   slab_abs[s] = |dy[Ts]|^T |x[Ts]|     bias[s] = sum_{Ts} dy   bias_abs[s] = sum_{Ts} |dy|
    w0 = sum_s slab[s], w1 = w0 + old_w;  b0 = sum_s bias[s], b1 = b0 + old_b     (the reduce with accumulate 0 / 1)
`exact_colsum(src, R, C, old)`: ref = old + sum_{r < R} src[r, :C] and abs = |old| + sum |src|.

Bounds (elementwise, derived, no fitted constant)
-------------------------------------------------
 slab s.  Both kernels add the exact products dy[m][n] x[m][k] with v_mfma_f32_32x32x16_bf16, 16 tokens per instruction, the four 16-token chunks
   kc = 0 .. 3 of a K-tile in order, K-tile after K-tile (gemm_tn.hip:142-153 and :309-317 -- the second kernel issues the same instructions on the same
   fragments per accumulator in the same order, gemm_tn.hip:184).  The last K-tile of the token range is always a whole tile: tokens m >= M come from
   the zero row (gemm_tn.hip:88-93, :244-254) and add exact zeros.  With ASSUMPTION 1 of gemm_reference.py (every add inside and between the MFMAs
   budgeted at 2 f, the order inside an instruction unknown) a product passes at most n_acc(Kp) = Kp / 16 + 16 adds, Kp = 64 ceil(|Ts| / 64) the
   split's own token count rounded up to the K-tiles the kernel runs:
       tol_slab[s] = gamma2(n_acc(Kp)) slab_abs[s] + Kp T          (T per product: a product below the smallest normal may be flushed)
   The epilogue stores the f32 accumulator itself (EPI_SLAB_F32, alpha = 1: no further rounding).
 bias partial of split s (gemm_tn_pp_kernel::colsum, gemm_tn.hip:318-337, and the join :364-370).  Lane l of a fragment holds 8 consecutive tokens
   16 kc + 8 (l >> 5) + 0 .. 7 of feature 32 i + (l & 31); per K-tile and feature the lane runs 4 chunks x 4 v_dot2c_f32_bf16 = 16 instructions
   c <- a0 * 1 + a1 * 1 + c in one chain (gemm_tn.hip:328-335), K-tile after K-tile, then the two token halves meet in ONE f32 add
   (__shfl_xor(.., 32), gemm_tn.hip:367).
   ASSUMPTION 3 (`FDOT2_F_PER_ADD`): the internal rounding of v_dot2c_f32_bf16 is not documented.  The two products by 1.0 are exact; each of the
   instruction's two adds is budgeted at 2 f (truncation, as for the MFMAs).  A token then passes at most 2 x 16 nkt adds of its lane's chain
   (nkt = the split's K-tiles) and the join:
       tol_bias[s] = gammaX(32 nkt + 1) bias_abs[s] + Kp T,     gammaX(n) = c n f / (1 - c n f),  c = FDOT2_F_PER_ADD = 2  (= gamma2)
   (Measured on an MI355X, profiles/dw_reference.md: the worst bias partial sits at 0.002 of this bound and int_tagged is exact; the budget was not widened.)
 owl_slab_reduce (gemm.hip:424-442: a = old | 0, then a += slab[s] for s = 0 .. nsplit - 1; the tall form gemm.hip:449-477 -- nsplit >= 128 and
   n <= 32768 -- adds in another fixed order whose chains are shorter).  Exactly as gemm_reference.py bounds its slab path:
       tol_w = sum_s tol_slab[s] + gamma(nsplit + 1) (sum_s (|slab[s]| + tol_slab[s]) + |old|) + T        (the same for the bias with tol_bias)
 colsum_bf16_kernel (backward.hip:825-846) / colsum_f32_kernel (backward.hip:793-809).  A workgroup owns 256 rows; wave w adds rows r0 + w, r0 + w + 4,
   ... onto 0 in order (backward.hip:832-837 / :800-803): at most 64 adds; the four waves meet as (p0 + p1) + (p2 + p3) (backward.hip:844 / :808):
   2 adds; partials_reduce_kernel (backward.hip:15-41) over the gy = ceil(R / 256) row blocks: thread j adds blocks j, j + 16, ... onto 0
   (ceil(gy / 16) adds), the 16 thread sums are added in order (15 adds), then the old value (1 add, backward.hip:38).  All plain f32 adds, RNE:
       chain = min(64, ceil(min(R, 256) / 4)) + 2 + ceil(gy / 16) + 16,      tol = gamma(chain) (sum |src| + |old|) + chain T
   (bf16 -> f32 by a shift is exact, backward.hip:836.)
 transpose_colsum_kernel (backward.hip:720-772).  A workgroup owns 64 columns x 512 rows (row_tiles = 8, backward.hip:778): thread (lr, lc) adds rows
   lr, lr + 32 of each of the 8 row tiles onto 0 (backward.hip:743): 16 adds; the 32 values of a column are added serially (backward.hip:768): 32
   adds; partials_reduce over gy = ceil(R / 512) blocks as above:
       chain = 16 + 32 + ceil(gy / 16) + 16,      tol = gamma(chain) (sum |src| + |old|) + chain T
   The transpose itself moves bf16 bits: exact.

Exact-integer profile.  `int_tagged` draws dy in [-2, 2] and x in [-3, 3] (integers) and overlays a deterministic tag that depends on the token AND
the feature, so neither rows nor columns are exchangeable.  `exact_tn` / `exact_colsum` return `exact_ok` = every sum of absolute values (old value
included) is below 2^24: every partial sum in ANY order is then an integer below 2^24, every f32 add is exact, and the device result must EQUAL the
reference (`check_exact`) -- per slab, per bias partial and after the reduce.  `assert_exact_ok` is asserted for every such case.

Float profiles (under the bounds): `randn`; `cancel` -- the sign of dy alternates from one 16-token chunk to the next over (nearly) equal x rows, of
size 8: |slab| << slab_abs, a relative-to-result test would pass a wrong kernel; `one_hot_token` -- one nonzero token at `pos`
(`one_hot_positions`: first and last token of a split, first and last row of a K-tile, M - 1): a mis-attributed token is a wholly wrong slab.

`untouched_rows` covers slab[nsplit:] and bias_slab[nsplit:]; the GPU test holds the pad columns of the transposed operands and everything behind a
gradient with it or by value (the padded reducer writes a dense [n_out, n_in] destination: a reduce that walked the padded width instead would both miss
the reference and run past the gradient's end).  `check` / `untouched` are gemm_reference's (every element, no exclusions, NaN outside; bits outside the written region); `check_exact` compares values
for equality.  `emulate_tn` / `emulate_colsum` are f32 simulations of the kernels' order (K-tiles of 64, four chunks of 16, split by split, then the
reduce; the waves' row strides and joins) for the CPU test of the bounds (tests/test_dw_reference.py); they are NOT a reference for the GPU test.
"""
import torch

from tests.gemm_reference import F, TINY, bf16_round, bits, check, gamma, gamma2, n_acc, untouched  # noqa: F401  (re-exported)

TBK = 64                    # tokens per K-tile                       gemm_tn.hip:23
CHUNK = 16                  # tokens per MFMA instruction
ROW_PAD = 128               # ops.pad_rows (tests/test_dw_reference.py holds it to ops.ROW_PAD)
FDOT2_F_PER_ADD = 2.0       # ASSUMPTION 3
EXACT_LIMIT = 2.0 ** 24
POISON_INT = 4096.0         # bf16-exact; one leaked pad element moves an int_tagged sum by a multiple of 4096


def cdiv(a, b):
    return (a + b - 1) // b


def pad_rows(n):
    return cdiv(n, ROW_PAD) * ROW_PAD


def gamma_x(n):
    """n chained adds budgeted at FDOT2_F_PER_ADD f each (the v_dot2c adds)."""
    return FDOT2_F_PER_ADD * n * F / (1.0 - FDOT2_F_PER_ADD * n * F)


def split_rule(M, splits):
    """-> (nk, per, nsplit, [(t0, t1)] token range of every split): gemm_tn.hip:405-408 restated."""
    nk = cdiv(M, TBK)
    splits = max(1, min(splits, nk))
    per = cdiv(nk, splits)
    ns = cdiv(nk, per)
    return nk, per, ns, [(TBK * per * s, min(M, TBK * per * (s + 1))) for s in range(ns)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact + bounds: the TN GEMM, its bias fold, the reduce
# ---------------------------------------------------------------------------------------------------------------------------------------------
def exact_tn(dy, x, rows, n_out, n_in, splits, old_w=None, old_b=None):
    """float64 reference (module docstring) -> dict."""
    Y, X = dy[:rows, :n_out].double(), x[:rows, :n_in].double()
    nk, per, ns, ranges = split_rule(rows, splits)
    Ya, Xa = Y.abs(), X.abs()
    r = {"rows": rows, "n_out": n_out, "n_in": n_in, "nk": nk, "per": per, "ns": ns, "ranges": ranges}
    r["slab"] = torch.stack([Y[a:b].t() @ X[a:b] for a, b in ranges])
    r["slab_abs"] = torch.stack([Ya[a:b].t() @ Xa[a:b] for a, b in ranges])
    r["bias"] = torch.stack([Y[a:b].sum(0) for a, b in ranges])
    r["bias_abs"] = torch.stack([Ya[a:b].sum(0) for a, b in ranges])
    r["w0"], r["b0"] = r["slab"].sum(0), r["bias"].sum(0)
    return set_old(r, old_w, old_b)


def set_old(r, old_w=None, old_b=None):
    """(Re)place the values the reduce adds into (accumulate 1) in a result of exact_tn: old_w, old_b, w1, b1, exact_ok."""
    r["old_w"] = torch.zeros_like(r["w0"]) if old_w is None else old_w.to(r["w0"].device).double()
    r["old_b"] = torch.zeros_like(r["b0"]) if old_b is None else old_b.to(r["b0"].device).double()
    r["w1"], r["b1"] = r["w0"] + r["old_w"], r["b0"] + r["old_b"]
    r["exact_ok"] = bool(float((r["slab_abs"].sum(0) + r["old_w"].abs()).max()) < EXACT_LIMIT
                         and float((r["bias_abs"].sum(0) + r["old_b"].abs()).max()) < EXACT_LIMIT)
    return r


def bounds_tn(r):
    """Elementwise tolerances for exact_tn's result: slab [ns, n_out, n_in], bias [ns, n_out], w0 / w1 [n_out, n_in], b0 / b1 [n_out]."""
    ts, tb = [], []
    for (a, b), sa, ba in zip(r["ranges"], r["slab_abs"], r["bias_abs"]):
        nkt = cdiv(b - a, TBK)
        Kp = nkt * TBK
        ts.append(gamma2(n_acc(Kp)) * sa + Kp * TINY)
        tb.append(gamma_x(2 * CHUNK * nkt + 1) * ba + Kp * TINY)
    ts, tb = torch.stack(ts), torch.stack(tb)
    g = gamma(r["ns"] + 1)
    mag_w, mag_b = (r["slab"].abs() + ts).sum(0), (r["bias"].abs() + tb).sum(0)
    return {"slab": ts, "bias": tb,
            "w0": ts.sum(0) + g * mag_w + TINY, "w1": ts.sum(0) + g * (mag_w + r["old_w"].abs()) + TINY,
            "b0": tb.sum(0) + g * mag_b + TINY, "b1": tb.sum(0) + g * (mag_b + r["old_b"].abs()) + TINY}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact + bounds: the column-sum kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
def reduce_chain(nblk):
    """adds a partial passes in partials_reduce_kernel with accumulate = 1 (backward.hip:25-38)."""
    return cdiv(nblk, 16) + 15 + 1


def colsum_chain(kind, R):
    """adds one input element passes on its way into the column sum: kind 'bf16' | 'f32' (colsum_*_kernel) or 'transpose' (transpose_colsum_kernel)."""
    if kind in ("bf16", "f32"):
        return min(64, cdiv(min(R, 256), 4)) + 2 + reduce_chain(cdiv(R, 256))
    if kind == "transpose":
        return 16 + 32 + reduce_chain(cdiv(R, 512))
    raise ValueError(kind)


def exact_colsum(src, R, C, old):
    S = src[:R, :C].double()
    r = {"ref": S.sum(0) + old.double(), "abs": S.abs().sum(0) + old.double().abs()}
    r["exact_ok"] = bool(float(r["abs"].max()) < EXACT_LIMIT)
    return r


def bounds_colsum(kind, R, r):
    n = colsum_chain(kind, R)
    return gamma(n) * r["abs"] + n * TINY


# ---------------------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------------------
def assert_exact_ok(r, what=""):
    assert r["exact_ok"], f"{what}: a sum of absolute values reaches 2^24 -- the exact-integer profile is not exact at this case"


def check_exact(name, got, ref, fails=None):
    """Every element of `got` EQUALS `ref` (values: -0 == +0, NaN equals nothing).  Returns the number of mismatches; on a mismatch raises -- or, given
    a list `fails`, appends the message -- with the count and the first indices (the tags of int_tagged make the token / feature pattern readable)."""
    bad = ~(got.double() == ref)
    nb = int(bad.sum())
    if nb:
        first = [f"{idx}: got {float(got[tuple(idx)]):.9g} ref {float(ref[tuple(idx)]):.9g}" for idx in bad.nonzero()[:8].tolist()]
        msg = f"{name}: {nb}/{bad.numel()} not equal to the float64 reference; " + "; ".join(first)
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)
    return nb


def untouched_rows(name, buf, before, nvalid, fails=None):
    """`buf` [n, ...] of which a call may write [0, nvalid) only: every later row holds its exact bits (slab[nsplit:], bias_slab[nsplit:])."""
    return untouched(name, buf.reshape(buf.shape[0], -1), before.reshape(before.shape[0], -1), nvalid, 0, buf[0].numel(), fails)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input profiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _gen(seed, *dims):
    s = seed * 1000003
    for d in dims:
        s = s * 10007 + d
    return torch.Generator(device="cpu").manual_seed(s % (2 ** 62))


def int_tagged(R, C, lim, seed):
    """[R, C] integers in [-lim, lim]: seeded draws, every (m + 3 c) % 5 == 0 element replaced by the tag (2 m + c) % (2 lim + 1) - lim."""
    v = torch.randint(-lim, lim + 1, (R, C), generator=_gen(seed, R, C, lim)).float()
    m = torch.arange(R).view(R, 1)
    c = torch.arange(C).view(1, C)
    tag = ((2 * m + c) % (2 * lim + 1) - lim).float()
    return torch.where((m + 3 * c) % 5 == 0, tag, v)


def poisoned(buf, rows, width, value):
    """A copy of `buf` with the pad rows [rows, ..) and the pad columns [width, ld) set to `value`."""
    out = buf.clone()
    out[rows:] = value
    out[:, width:] = value
    return out


def make_inputs(profile, rows, n_out, n_in, seed=1, ldy=None, ldx=None, poison=float("nan"), pos=None):
    """Seeded bf16-exact operands on the CPU (float32): dy [pad_rows(rows), ldy], x [pad_rows(rows), ldx]; pad rows and pad columns hold `poison`."""
    ldy, ldx = ldy or n_out, ldx or n_in
    g = _gen(seed, rows, n_out, n_in)
    if profile == "int_tagged":
        Y, X = int_tagged(rows, n_out, 2, seed), int_tagged(rows, n_in, 3, seed + 1)
    elif profile == "randn":
        Y, X = torch.randn(rows, n_out, generator=g), torch.randn(rows, n_in, generator=g)
    elif profile == "cancel":
        nch = cdiv(rows, 2 * CHUNK)
        base_y = torch.randn(nch, CHUNK, n_out, generator=g) * 8.0
        base_x = torch.randn(nch, CHUNK, n_in, generator=g)
        Y = torch.stack([base_y, -base_y], 1).reshape(-1, n_out)[:rows]
        X = torch.stack([base_x, base_x * (1.0 + 2.0 ** -6 * torch.randn(nch, CHUNK, n_in, generator=g))], 1).reshape(-1, n_in)[:rows]
    elif profile == "one_hot_token":
        Y, X = torch.zeros(rows, n_out), torch.zeros(rows, n_in)
        Y[pos], X[pos] = torch.randn(n_out, generator=g), torch.randn(n_in, generator=g)
    else:
        raise ValueError(profile)
    dy = torch.full((pad_rows(rows), ldy), poison)
    x = torch.full((pad_rows(rows), ldx), poison)
    dy[:rows, :n_out], x[:rows, :n_in] = bf16_round(Y), bf16_round(X)
    return dy, x


def make_old(profile, ref, seed=1):
    """The value the reduce adds into (accumulate 1): integers for int_tagged, else of the gradient's own size."""
    g = _gen(seed, *ref.shape)
    ref = ref.cpu()
    if profile == "int_tagged":
        return torch.randint(-1000, 1001, tuple(ref.shape), generator=g).float()
    return torch.randn(tuple(ref.shape), generator=g) * max(float(ref.abs().mean()), 2.0 ** -20)


def one_hot_positions(rows, splits):
    """Tokens for `one_hot_token`: first / last token of a middle split, the last token of the split before it, the first of the last split, first / last row of a K-tile inside a split, the last
    row of the last whole K-tile, M - 1."""
    nk, per, ns, ranges = split_rule(rows, splits)
    a, b = ranges[ns // 2]
    kt = min(nk - 1, per * (ns // 2) + (1 if per > 1 else 0))
    pos = {max(a - 1, 0), a, b - 1, ranges[-1][0], rows - 1, TBK * kt, min(rows, TBK * kt + TBK) - 1}
    if rows >= TBK:
        pos.add(TBK * (rows // TBK) - 1)
    return sorted(pos)


def make_colsum_input(profile, kind, R, C, seed=1, ld=None, poison=float("nan"), rows_alloc=None):
    """[rows_alloc or R + 3, ld] f32 (kind 'f32') or bf16-exact values (else); rows >= R and columns >= C hold `poison`."""
    ld = ld or C
    g = _gen(seed, R, C, 7)
    if profile == "int_tagged":
        S = int_tagged(R, C, 3, seed)
    elif profile == "randn":
        S = torch.randn(R, C, generator=g)
    elif profile == "cancel":
        half = torch.randn(cdiv(R, 2), C, generator=g) * 8.0
        S = torch.stack([half, -half * (1.0 + 2.0 ** -6 * torch.randn(half.shape, generator=g))], 1).reshape(-1, C)[:R]
    else:
        raise ValueError(profile)
    buf = torch.full((rows_alloc or R + 3, ld), poison)
    buf[:R, :C] = S if kind == "f32" else bf16_round(S)
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------------------
# f32 simulation of the kernels' order (CPU test only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def emulate_tn(dy, x, rows, n_out, n_in, splits, old_w=None, old_b=None, hooks=None):
    """f32 simulation of one owl_gemm_tn_slab_bf16 call with a bias slab and of the two owl_slab_reduce calls (module docstring) -> dict slab, bias,
    w0, w1, b0, b1.  `hooks` lets a test plant an error:
      "stage"(kt, Y, X) -> (Y, X)    the LDS image [64, n_out], [64, n_in] of K-tile kt (rows m >= M are zero rows)
      "walk"(s, kts) -> kts          the K-tiles split s reads, in order (slab and bias fold alike: the fold adds the MFMAs' own fragments)
      "bias_walk"(s, kts) -> kts     the K-tiles the bias fold of split s reads
      "fold_pairs"                   the token pairs of a fragment the fold adds (default (0, 1, 2, 3))
      "slab"(s, acc) -> acc          the stored slab"""
    hooks = hooks or {}
    dy, x = dy.float(), x.float()
    nk, per, ns, _ = split_rule(rows, splits)
    pairs = hooks.get("fold_pairs", (0, 1, 2, 3))

    def stage(kt):
        Y, X = torch.zeros(TBK, n_out), torch.zeros(TBK, n_in)
        v = max(0, min(TBK, rows - kt * TBK))
        Y[:v], X[:v] = dy[kt * TBK: kt * TBK + v, :n_out], x[kt * TBK: kt * TBK + v, :n_in]
        return hooks["stage"](kt, Y, X) if "stage" in hooks else (Y, X)

    slabs, biases = [], []
    for s in range(ns):
        kts = list(range(s * per, min(nk, (s + 1) * per)))
        kts = hooks["walk"](s, kts) if "walk" in hooks else kts
        acc = torch.zeros(n_out, n_in)
        for kt in kts:
            Y, X = stage(kt)
            for kc in range(TBK // CHUNK):
                acc = acc + Y[kc * CHUNK:(kc + 1) * CHUNK].t() @ X[kc * CHUNK:(kc + 1) * CHUNK]
        cs = torch.zeros(2, n_out)                      # the two token halves (lanes l, l + 32) of every feature
        for kt in (hooks["bias_walk"](s, kts) if "bias_walk" in hooks else kts):
            Y, _ = stage(kt)
            for kc in range(TBK // CHUNK):
                for h in range(2):
                    frag = Y[kc * CHUNK + 8 * h: kc * CHUNK + 8 * h + 8]
                    for p in pairs:
                        cs[h] = (cs[h] + frag[2 * p]) + frag[2 * p + 1]
        slabs.append(hooks["slab"](s, acc) if "slab" in hooks else acc)
        biases.append(cs[0] + cs[1])
    out = {"slab": torch.stack(slabs), "bias": torch.stack(biases)}
    for key, parts, old in (("w", out["slab"], old_w), ("b", out["bias"], old_b)):
        for accumulate in (0, 1):
            a = old.float().clone() if (accumulate and old is not None) else torch.zeros_like(parts[0])
            for p in parts:
                a = a + p
            out[f"{key}{accumulate}"] = a
    return out


def _emulate_partials_reduce(parts, old):
    red = []
    for j in range(16):
        a = torch.zeros_like(parts[0])
        for s in range(j, len(parts), 16):
            a = a + parts[s]
        red.append(a)
    t = red[0]
    for k in range(1, 16):
        t = t + red[k]
    return t + old.float()


def emulate_colsum(kind, src, R, C, old):
    """f32 simulation of owl_colsum_bf16 / owl_colsum_f32 ('bf16' / 'f32') or of owl_transpose_colsum_bf16's column sums ('transpose')."""
    S = src[:R, :C].float()
    parts = []
    if kind in ("bf16", "f32"):
        for r0 in range(0, R, 256):
            blk = S[r0:r0 + 256]
            p = []
            for w in range(4):
                a = torch.zeros(C)
                for row in blk[w::4]:
                    a = a + row
                p.append(a)
            parts.append((p[0] + p[1]) + (p[2] + p[3]))
    elif kind == "transpose":
        for r0 in range(0, R, 512):
            blk = torch.zeros(512, C)
            blk[:min(512, R - r0)] = S[r0:r0 + 512]
            acc = torch.zeros(32, C)
            for step in range(16):
                acc = acc + blk[32 * step: 32 * step + 32]
            s = torch.zeros(C)
            for k in range(32):
                s = s + acc[k]
            parts.append(s)
    else:
        raise ValueError(kind)
    return _emulate_partials_reduce(parts, old)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case set shared by the CPU and the GPU test
# ---------------------------------------------------------------------------------------------------------------------------------------------
# (rows, splits): what the largest kt_per_split and the tail reach
ROW_CASES = [(5, 1),          # one partial K-tile only
             (384, 1),        # 6 full K-tiles; never the zero-row path
             (357, 1),        # 6 K-tiles; the last has 37 valid rows
             (357, 2),        # per = 3; the tail sits in a 3-tile split
             (385, 3),        # nk = 7, per = 3, nsplit = 3; the last split is ONE K-tile holding ONE valid row
             (129, 8)]        # the split request is clamped (nk = 3); slab[nsplit:] untouched
# (n_out, n_in)
WIDTHS = [(256, 256),         # baseline, one tile
          (512, 256),         # two n tiles
          (256, 512),         # two k tiles; tk = 1 does no bias fold
          (264, 328),         # ragged second tiles: 8 and 72 valid columns
          (40, 256),          # small-n_out clamp
          (8, 256),           # minimum n_out
          (32, 512)]          # the routed prompt-gradient form
# The reduction of WIDTHS x ROW_CASES: the baseline width meets every row case; every other width meets the two row cases that hold the whole stream
# inside one work item -- (357, 2): three K-tiles and the tail in one split; (385, 3): three K-tiles per split and the one-row tail -- the ragged width
# also the clamped request.  The row cases differ in the token walk only, which no width changes (gemm_tn.hip:206-212: tile and split are decoded
# independently).
WIDE_ROW_CASES = [(357, 2), (385, 3)]
PERSISTENT = (5605, 44, 768, 512)          # rows, splits, n_out, n_in: nk = 88, per = 2, 6 tiles x 44 splits = 264 items > 256 (gemm_tn.hip:425)
LD_CASE = (357, 2, 256, 256, 264, 328)     # rows, splits, n_out, n_in, ldy, ldx: operands wider than the product reads, as the patch operand is


def tn_cases():
    """[(rows, splits, n_out, n_in, ldy, ldx)]"""
    out = [(r, s, 256, 256, 256, 256) for r, s in ROW_CASES]
    for n_out, n_in in WIDTHS[1:]:
        rc = WIDE_ROW_CASES + ([(129, 8)] if (n_out, n_in) == (264, 328) else [])
        out += [(r, s, n_out, n_in, n_out, n_in) for r, s in rc]
    out.append(LD_CASE)
    return out


def n_items(rows, splits, n_out, n_in):
    return cdiv(n_out, 256) * cdiv(n_in, 256) * split_rule(rows, splits)[2]


COLSUM_R = (1, 3, 255, 256, 257, 1029)     # 1029: 5 row blocks into partials_reduce
COLSUM_C = {"bf16": (8, 512, 520), "f32": (4, 256, 260)}
COLSUM_LD = (257, 520, 528)                # one bf16 case with ld > C
TRANSPOSE_R = (8, 203, 512, 523)           # 203: the scalar store tail; 523: grid.y = 2 with a ragged second block
TRANSPOSE_C = (64, 72, 136)
TRANSPOSE_ONLY_C = 588                     # no column sums (C % 8 != 0 chunk at the end: the `c + 8 > C` scalar load path)
