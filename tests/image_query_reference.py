"""Float64 reference, derived error bounds, input profiles and an order-faithful CPU emulation for csrc/image_query.hip (owl_image_query_select,
owl_query_bank_fill).  Checker side; device-agnostic; nothing here imports the package's Python ops.

Reference
---------
`exact_select(e, boxes, qbox)`, one exemplar: the float64 restatement of HF `embed_image_query` (HF5 modeling_owlvit.py:1246-1288) on the kernel's exact
f32 inputs, the IoU stage evaluated in float64 too:
  1. iou_p = box_iou(qbox, boxes_p);  2. every iou_p == 0 -> v_p = iou_p - (hull_p - union_p) / hull_p, else v_p = iou_p;
  3. thr = max_p v_p * fl32(0.8), selected = {v_p >= thr} (a negative maximum selects nothing: EMPTY, where HF drops the image);
  4. mean_k = sum over ALL p of e[p, k] / P;  5. sim_p = mean . e[p];  6. best = the first minimum of sim over the selected.
It returns the per-box threshold margins |v_p - thr| and the argmin margin (second smallest - smallest selected sim).
`exact_bank(query, table)`: bank[r] = unit(sum over table[r], ascending, of unit(query_m)) in float64.

Bounds (elementwise, derived, no fitted constant).  F = 2^-24, U64 = 2^-53, gamma as gemm_reference.py; _V (one rounding per written operation) is
layernorm_reference.py:303-326, the division heads_reference._div under its ASSUMPTION H1 (the f32 division within 2 ulp).
  v_p     the kernel's chain, contraction off: area_q, area_p = (x1 - x0)(y1 - y0): 3 roundings each; lt, rb exact (max / min of exact inputs);
          wh = clamp(rb - lt, 0): 1 each; inter = w h: 1; union = (area_q + area_p) - inter: 2; iou = inter / union: H1.  Fallback: hull corners exact,
          wh 1 each, hull = w h: 1, hull - union: 1, / hull: H1, iou - .: 1.  All carried by _V, so cancellation in `hull - union` is charged at the
          operands' size.  `E_v`.  Not charged: an f32 UNDERFLOW of a positive product to 0 (sides below 2^-60 -- no profile goes there).
  thr     |max~ - max| <= max_p E_v (the error of a maximum is at most the largest error), one multiply by the exact f32 0.8f: `E_thr`.
  mean_k  f64, in the order the kernel uses: 64 adds inside a row block (image_query_colsum_kernel), ceil(P / 64) adds over the blocks, one division
          (charged 2): n_mean = 64 + ceil(P / 64) + 2;  E_mean = gamma64(n_mean) sum_p |e[p, k]| / P.
  sim_p   lane chain 4 ceil(Dt / 256) FMAs + 6 butterfly levels, + 1 so that an unfused multiply-add (the CPU emulation) is covered too:
          n_dot = 4 ceil(Dt / 256) + 7;  E_sim = sum_k |e[p, k]| E_mean_k + gamma64(n_dot) sum_k (|mean_k| + E_mean_k) |e[p, k]|.
  bank    one f32 rounding of an f64 value whose own error is gamma64(2 (Dt + members) + 16) of its size: tol = F |ref| + that + TINY.

Decisions (`check_select`).  Membership of p must equal the reference's wherever |v_p - thr| > E_v + E_thr, and may go either way elsewhere (S = the
decided members, A = S + the undecided boxes).  best must lie in A with sim_ref[best] - sim_ref[p] <= E_best + E_p for every p in S, and must be the
FIRST minimum of the kernel's own sim_out (the lowest index on exact ties).  An exemplar is DECIDED when every membership is decided and the
reference's best beats every other member by more than the two bounds; then best must be the reference's.  query == e[best] bit for bit.

Profiles (`make_case`): randn, ties, touching, disjoint, near_thr, offset -- see each branch.  tests/test_image_query_reference.py asserts that each
reaches what it names and that the caps hold (randn: every exemplar decided; near_thr / offset: at most a quarter undecided).

`emulate_select` follows the kernel's order on the CPU (f32 IoU chain one torch op per written operation, f64 sums in the kernel's order) and takes
`hooks` that plant errors; CPU test only, NEVER a reference on the GPU.
"""

import torch

from tests.gemm_reference import F, TINY, check, gamma as gam, ratios  # noqa: F401
from tests.heads_reference import _div
from tests.layernorm_reference import _V

U64 = 2.0 ** -53
ROWS = 64                     # IQ_ROWS of csrc/image_query.hip
C08 = float(torch.tensor(0.8, dtype=torch.float32))
INF = float("inf")
FLAG_FALLBACK, FLAG_EMPTY = 1, 2
WHOLE = (0.0, 0.0, 1.0, 1.0)

GPU_CASES = [(1, 1, 64, "randn"), (3, 36, 64, "touching"), (3, 36, 64, "disjoint"), (3, 36, 64, "ties"), (70, 36, 64, "randn"),
             (5, 577, 512, "near_thr"), (5, 577, 512, "ties"), (2, 2304, 512, "randn"), (2, 2304, 512, "offset"), (2, 3600, 768, "randn"),
             (2, 3600, 768, "offset"), (1, 8192, 768, "randn"), (1, 8192, 768, "ties")]
UNDECIDED_CAP = {"randn": 0.0, "near_thr": 0.25, "offset": 0.25}          # largest share of exemplars the bounds may leave undecided


def cdiv(a, b):
    return (a + b - 1) // b


def gam64(n):
    return n * U64 / (1.0 - n * U64)


def n_mean(P):
    return ROWS + cdiv(P, ROWS) + 2


def n_dot(Dt):
    return 4 * cdiv(Dt, 256) + 7


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _iou_V(q, b, Eb=0.0):
    """(iou, union) as _V over the P boxes b [P, 4] (f64 of the f32 inputs) against the query box q [4].  Eb: what every box coordinate the kernel is
    handed may differ by from b (0 for the kernel tests; the model-level test's bf16 forward error); a min / max errs by at most its operands' largest error."""
    Eb = torch.full_like(b[:, 0], float(Eb))
    qx0, qy0, qx1, qy1 = (_V(q[i].expand(b.shape[0]).clone()) for i in range(4))
    bx0, by0, bx1, by1 = (_V(b[:, i].clone(), Eb.clone()) for i in range(4))
    area_q = (qx1 - qx0) * (qy1 - qy0)
    area_p = (bx1 - bx0) * (by1 - by0)
    w = _V(torch.minimum(qx1.v, bx1.v), Eb.clone()) - _V(torch.maximum(qx0.v, bx0.v), Eb.clone())
    h = _V(torch.minimum(qy1.v, by1.v), Eb.clone()) - _V(torch.maximum(qy0.v, by0.v), Eb.clone())
    w, h = _V(w.v.clamp(min=0), w.E), _V(h.v.clamp(min=0), h.E)
    inter = w * h
    union = (area_q + area_p) - inter
    return _div(inter, union), union


def _giou_V(q, b, Eb=0.0):
    iou, union = _iou_V(q, b, Eb)
    Eb = torch.full_like(b[:, 0], float(Eb))
    w = _V(torch.maximum(q[2], b[:, 2]), Eb.clone()) - _V(torch.minimum(q[0], b[:, 0]), Eb.clone())
    h = _V(torch.maximum(q[3], b[:, 3]), Eb.clone()) - _V(torch.minimum(q[1], b[:, 1]), Eb.clone())
    w, h = _V(w.v.clamp(min=0), w.E), _V(h.v.clamp(min=0), h.E)
    hull = w * h
    return iou - _div(hull - union, hull)


def exact_select(e, boxes, qbox=None, E_e=0.0, E_box=0.0):
    """One exemplar: e f32 [P, Dt], boxes f32 [P, 4], qbox f32 [4] or None (the whole image).  -> dict of float64 values, bounds and margins.
    E_e / E_box (0 for the kernel tests): the inputs the kernel is handed may differ from e / boxes by that much, elementwise -- the model-level test
    hands in the ORACLE's e and boxes with the bf16 forward's tolerances, and the bounds, hence `decided`, then say which decisions survive that; a
    fallback decision that box errors could flip (some iou's bound reaches 0 either way) is then undecided."""
    P, Dt = e.shape
    e64, b = e.double(), boxes.double()
    q = torch.tensor(WHOLE, dtype=torch.float64, device=e.device) if qbox is None else qbox.double()
    iou, _ = _iou_V(q, b, E_box)
    fallback = bool((iou.v == 0).all())
    v = _giou_V(q, b, E_box) if fallback else iou
    vmax = v.v.max()
    thr = vmax * C08
    E_thr = C08 * v.E.max() + F * (thr.abs() + C08 * v.E.max()) + TINY
    sel = v.v >= thr
    margin_v = (v.v - thr).abs()
    decided_mem = margin_v > v.E + E_thr
    mean = e64.sum(0) / P
    E_mean = gam64(n_mean(P)) * e64.abs().sum(0) / P
    sim = e64 @ mean
    E_sim = e64.abs() @ E_mean + gam64(n_dot(Dt)) * (e64.abs() @ (mean.abs() + E_mean))
    sure_fallback = True
    if E_e or E_box:          # |m~ . e~ - m . e| <= sum_k |m_k| E_e + (|e_k| + E_e) E_m, E_m = E_mean + E_e (the mean of values off by E_e is off by E_e)
        E_mean = E_mean + E_e
        E_sim = E_sim + E_e * mean.abs().sum() + (e64.abs() + E_e) @ E_mean
        sure_fallback = bool((iou.v > iou.E).any()) if not fallback else False
    out = dict(P=P, Dt=Dt, fallback=fallback, v=v.v, E_v=v.E, thr=thr, E_thr=E_thr, sel=sel, margin_v=margin_v, decided_mem=decided_mem, mean=mean,
               E_mean=E_mean, sim=sim, E_sim=E_sim, nsel=int(sel.sum()), empty=not bool(sel.any()))
    if not sure_fallback:
        decided_mem = torch.zeros_like(decided_mem)
        out["decided_mem"] = decided_mem
    if out["empty"]:
        out.update(best=-1, margin_best=INF, decided=bool(decided_mem.all()))
        return out
    idx = sel.nonzero().flatten()
    s = sim[idx]
    j = int(torch.argmin(s))          # the first minimum
    best = int(idx[j])
    others = torch.ones_like(s, dtype=torch.bool)
    others[j] = False
    if bool(others.any()):
        gap = (s[others] - s[j]) - (E_sim[idx][others] + E_sim[best])
        out.update(margin_best=float((s[others] - s[j]).min()), decided=bool(decided_mem.all()) and bool((gap > 0).all()))
    else:
        out.update(margin_best=INF, decided=bool(decided_mem.all()))
    out["best"] = best
    return out


def exact_bank(query, table, old):
    """float64 bank [rows, Dt] (rows without members = old) and its tolerance."""
    q = query.double()
    unit = q / torch.linalg.norm(q, dim=-1, keepdim=True)
    ref = old.double().clone()
    tol = torch.zeros_like(ref)
    Dt = q.shape[1]
    for r, mem in enumerate(table):
        if not mem:
            continue
        s = unit[mem].sum(0)
        ref[r] = s / torch.linalg.norm(s)
        tol[r] = F * ref[r].abs() + gam64(2 * (Dt + len(mem)) + 16) * (1.0 + ref[r].abs()) + TINY
    return ref, tol


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the check shared by the CPU emulation and the GPU kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
def check_select(name, out, ref, e, fails=None):
    """out: dict(best int, query [Dt], flags int, nsel int, v [P], mean [Dt], sim [P]) of ONE exemplar, ref = exact_select of its inputs.  Appends
    messages to `fails` (or raises) -> dict of the worst err / tol per quantity."""
    own = [] if fails is None else fails
    n0 = len(own)
    r_v = check(f"{name} v", out["v"].cpu(), ref["v"].cpu(), ref["E_v"].cpu(), own)
    r_m = check(f"{name} mean", out["mean"].cpu(), ref["mean"].cpu(), ref["E_mean"].cpu() + TINY, own)
    got_sel = torch.isfinite(out["sim"]).cpu()
    sim_k = out["sim"].cpu()
    dm, rs = ref["decided_mem"].cpu(), ref["sel"].cpu()
    wrong = dm & (got_sel != rs)
    if bool(wrong.any()):
        p = int(wrong.nonzero()[0])
        own.append(f"{name}: membership of {int(wrong.sum())} decided boxes differs, first p = {p}: kernel {bool(got_sel[p])}, reference {bool(rs[p])} "
                   f"(v {float(ref['v'][p]):.9g}, thr {float(ref['thr']):.9g}, bound {float(ref['E_v'][p] + ref['E_thr']):.3g})")
    r_s = 0.0
    if bool(got_sel.any()):
        r_s = check(f"{name} sim", sim_k[got_sel], ref["sim"].cpu()[got_sel], ref["E_sim"].cpu()[got_sel] + TINY, own)
    if int(got_sel.sum()) != out["nsel"]:
        own.append(f"{name}: info says {out['nsel']} selected, sim_out marks {int(got_sel.sum())}")
    if bool(out["flags"] & FLAG_FALLBACK) != ref["fallback"]:
        own.append(f"{name}: fallback flag {bool(out['flags'] & FLAG_FALLBACK)}, reference {ref['fallback']}")
    best = out["best"]
    if bool(out["flags"] & FLAG_EMPTY) != (best < 0) or (best < 0) != (out["nsel"] == 0):
        own.append(f"{name}: best {best}, flags {out['flags']}, nsel {out['nsel']} disagree about emptiness")
    S, A = dm & rs, rs | ~dm
    if best < 0:
        if bool(S.any()):
            own.append(f"{name}: reported empty, the reference selects {int(S.sum())} boxes decidedly")
        if bool((out["query"] != 0).any()):
            own.append(f"{name}: an empty exemplar's query is not all zero")
    else:
        if not bool(A[best]):
            own.append(f"{name}: best = {best} is decidedly not selected by the reference")
        if bool(S.any()):
            sim, E = ref["sim"].cpu(), ref["E_sim"].cpu()
            over = (sim[best] - sim[S]) - (E[best] + E[S])
            if bool((over > 0).any()):
                own.append(f"{name}: sim_ref[best = {best}] = {float(sim[best]):.12g} exceeds a decided member's by {float(over.max()):.3g} beyond the bounds "
                           f"(reference best {ref['best']}: {float(sim[ref['best']]):.12g})")
        if bool(got_sel.any()):
            first = int(torch.argmin(torch.where(got_sel, sim_k, torch.full_like(sim_k, INF))))
            if first != best:
                own.append(f"{name}: best = {best} is not the first minimum of the kernel's own sims ({first}: {float(sim_k[first]):.17g} vs {float(sim_k[best]):.17g})")
        if not torch.equal(out["query"].cpu(), e[best].cpu()):
            own.append(f"{name}: query is not e[best] bit for bit")
    if ref["decided"] and best != ref["best"]:
        own.append(f"{name}: decided exemplar: best = {best}, reference {ref['best']} (argmin margin {ref['margin_best']:.3g})")
    if fails is None and len(own) > n0:
        raise AssertionError("; ".join(own[n0:]))
    return dict(v=r_v, mean=r_m, sim=r_s)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# profiles
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _corners(g, n):
    c = torch.sigmoid(torch.randn(n, 4, generator=g))
    return torch.stack([c[:, 0] - c[:, 2] / 2, c[:, 1] - c[:, 3] / 2, c[:, 0] + c[:, 2] / 2, c[:, 1] + c[:, 3] / 2], 1)


def _right_half(g, n):
    """boxes strictly inside x > 0.55: disjoint from, and not touching, any query box with x1 <= 0.5"""
    x0 = 0.6 + 0.2 * torch.rand(n, generator=g)
    y0 = 0.1 + 0.5 * torch.rand(n, generator=g)
    return torch.stack([x0, y0, x0 + 0.05 + 0.1 * torch.rand(n, generator=g), y0 + 0.05 + 0.3 * torch.rand(n, generator=g)], 1)


SEEDS = {}          # (profile, N, P, Dt) -> seed, where the default (0) does not meet the profile's cap


def make_case(profile, N, P, Dt, seed=None):
    """-> e f32 [N, P, Dt], boxes f32 [N, P, 4], qbox f32 [N, 4]."""
    seed = SEEDS.get((profile, N, P, Dt), 0) if seed is None else seed
    g = torch.Generator().manual_seed(1000 * seed + 7 * P + Dt + N + sum(map(ord, profile)))
    e = 0.7 * torch.randn(N, P, Dt, generator=g)
    boxes = _corners(g, N * P).view(N, P, 4)
    qbox = torch.tensor(WHOLE).repeat(N, 1)
    if profile == "randn":
        # e = 0.7 randn, boxes = corners of sigmoid(randn); odd exemplars: a random query box of side 0.1 .. 0.4, even ones: the whole image
        for n in range(1, N, 2):
            s = 0.1 + 0.3 * torch.rand(2, generator=g)
            o = torch.rand(2, generator=g) * (1 - s)
            qbox[n] = torch.cat([o, o + s])
    elif profile == "ties":
        # every box identical -> everything is selected; rows duplicated in pairs -> every sim, the minimum included, is tied exactly
        boxes[:] = torch.tensor([0.2, 0.25, 0.8, 0.75])
        e[:, 1::2] = e[:, 0:2 * (P // 2):2]
    elif profile == "touching":
        # query [0, 0, .5, 1]; box P // 3 = [.5, 0, 1, 1] touches it exactly (gIoU 0, every number exact); the others are disjoint: fallback, one selected
        qbox[:] = torch.tensor([0.0, 0.0, 0.5, 1.0])
        boxes = _right_half(g, N * P).view(N, P, 4)
        boxes[:, P // 3] = torch.tensor([0.5, 0.0, 1.0, 1.0])
    elif profile == "disjoint":
        # nothing overlaps or touches: the fallback's maximum is negative -> empty
        qbox[:] = torch.tensor([0.0, 0.0, 0.3, 0.3])
        boxes = _right_half(g, N * P).view(N, P, 4)
    elif profile == "near_thr":
        # whole-image query: iou = the box's area.  Box 0 = the maximum (area A = 0.64); boxes 1 .. 7 = [0, 0, w, 1] with w = 0.8 A moved by
        # (k - 4) ulp in every fifth exemplar (inside the bounds: either membership is accepted) and by 64 (k - 4) ulp in the others (near, but decided;
        # k = 4 sits 32 ulp above); the rest well below the threshold
        boxes = 0.5 * boxes.clamp(0, 1)
        boxes[:, 0] = torch.tensor([0.1, 0.1, 0.9, 0.9])
        a = float((torch.tensor(0.9) - torch.tensor(0.1)) ** 2)
        for n in range(N):
            for k in range(1, min(8, P)):
                steps = (k - 4) if n % 5 == 0 else (64 * (k - 4) or 32)
                w = torch.tensor(C08 * a, dtype=torch.float32)
                for _ in range(abs(steps)):
                    w = torch.nextafter(w, torch.tensor(INF if steps > 0 else -INF))
                boxes[n, k] = torch.stack([torch.tensor(0.0), torch.tensor(0.0), w, torch.tensor(1.0)])
    elif profile == "offset":
        # a large common vector + small noise: the sims are |c|^2 + O(noise) and nearly cancel in every comparison
        e = 30.0 * torch.randn(1, 1, Dt, generator=g) + 0.01 * torch.randn(N, P, Dt, generator=g)
        for n in range(1, N, 2):
            s = 0.1 + 0.3 * torch.rand(2, generator=g)
            o = torch.rand(2, generator=g) * (1 - s)
            qbox[n] = torch.cat([o, o + s])
    else:
        raise ValueError(profile)
    return e.contiguous(), boxes.contiguous(), qbox.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the kernel's order on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _iou32(q, b, hooks=()):
    area_q = (q[2] - q[0]) * (q[3] - q[1])
    area_p = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(q[2], b[:, 2]) - torch.maximum(q[0], b[:, 0])).clamp(min=0)
    h = (torch.minimum(q[3], b[:, 3]) - torch.maximum(q[1], b[:, 1])).clamp(min=0)
    inter = w * h
    union = (area_q + area_p) if "union_no_inter" in hooks else (area_q + area_p) - inter
    return inter / union, union


def emulate_select(e, boxes, qbox=None, hooks=()):
    """One exemplar in the kernel's arithmetic and order (f32 IoU chain, f64 sums).  hooks: thr075, argmax, mean_selected, tie_last, no_fallback,
    union_no_inter, f32_accum.  -> the dict check_select takes."""
    P, Dt = e.shape
    q = torch.tensor(WHOLE) if qbox is None else qbox.float()
    b = boxes.float()
    v, union = _iou32(q, b, hooks)
    fallback = bool((v == 0).all()) and "no_fallback" not in hooks
    if fallback:
        w = (torch.maximum(q[2], b[:, 2]) - torch.minimum(q[0], b[:, 0])).clamp(min=0)
        h = (torch.maximum(q[3], b[:, 3]) - torch.minimum(q[1], b[:, 1])).clamp(min=0)
        hull = w * h
        v = v - (hull - union) / hull
    thr = v.max() * torch.tensor(0.75 if "thr075" in hooks else 0.8, dtype=torch.float32)
    sel = v >= thr
    acc_t = torch.float32 if "f32_accum" in hooks else torch.float64
    RB = cdiv(P, ROWS)
    src = e[sel] if "mean_selected" in hooks else e
    n_src = src.shape[0]
    RBs = cdiv(max(n_src, 1), ROWS)
    pad = torch.zeros(RBs * ROWS, Dt, dtype=acc_t)
    pad[:n_src] = src.to(acc_t)
    pad = pad.view(RBs, ROWS, Dt)
    part = torch.zeros(RBs, Dt, dtype=acc_t)
    for i in range(ROWS):          # rows of a block in ascending order (adding a pad row's exact 0 changes nothing)
        part = part + pad[:, i]
    tot = torch.zeros(Dt, dtype=acc_t)
    for rb in range(RBs):
        tot = tot + part[rb]
    mean = tot / max(n_src, 1)
    idx = sel.nonzero().flatten()
    sim = torch.full((P,), INF, dtype=torch.float64)
    if idx.numel():
        rows = e[idx].to(acc_t)
        J = cdiv(Dt, 256)
        prod = torch.zeros(idx.numel(), J * 256, dtype=acc_t)
        prod[:, :Dt] = rows * mean
        prod = prod.view(-1, J, 64, 4)          # [row, j, lane, i]: lane l owns k = 256 j + 4 l + i
        acc = torch.zeros(idx.numel(), 64, dtype=acc_t)
        for j in range(J):
            for i in range(4):
                acc = acc + prod[:, j, :, i]
        o = 32
        while o:          # the butterfly: lane l += lane l ^ o
            acc = acc + acc[:, torch.arange(64) ^ o]
            o >>= 1
        sim[idx] = acc[:, 0].double()
    best = -1
    if idx.numel():
        s = sim[idx]
        if "argmax" in hooks:
            j = int(torch.argmax(s))
        elif "tie_last" in hooks:
            j = int((s == s.min()).nonzero()[-1])
        else:
            j = int(torch.argmin(s))
        best = int(idx[j])
    return dict(best=best, query=e[best].clone() if best >= 0 else torch.zeros(Dt), flags=(FLAG_FALLBACK if fallback else 0) | (FLAG_EMPTY if best < 0 else 0),
                nsel=int(idx.numel()), v=v, mean=mean.double(), sim=sim)


def undecided_share(profile, N, P, Dt):
    """(share of exemplars the bounds leave undecided, worst threshold margin, worst argmin margin) of make_case's default seed."""
    e, boxes, qbox = make_case(profile, N, P, Dt)
    refs = [exact_select(e[n], boxes[n], qbox[n]) for n in range(N)]
    und = sum(0 if r["decided"] else 1 for r in refs)
    return und / N, min(float(r["margin_v"].min()) for r in refs), min(r["margin_best"] for r in refs)
