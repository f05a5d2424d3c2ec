"""-m gpu: a call's bits do not depend on what an earlier call left in its scratch (profiles/history_independence.md).

Every row of ENTRIES names one exported entry that takes caller scratch or an in / out state buffer.  The row builds fixed inputs and calls the raw entry
(_lib.call) three times into freshly sentinel-filled outputs; the scratch of the three calls is

    zero     zero-filled;
    ones     every byte 0xFF: NaN as f32 / bf16 / f64, -1 as an integer -- a word read before it is written reaches an output as NaN or as a wild index;
    after    what a call of the same entry on another, LARGER problem (another seed, more rows, more partial blocks, more candidates, wider where the
             layout allows) left in the same allocation.

Asserted: every documented output bit-equal across the three; no NaN in an output (no input of any row implies one); the bytes behind the queried scratch
size untouched (a 0xA5 tail behind the probe's size under zero / ones, the predecessor's own leavings and the tail behind them under `after`); buffers the
header documents as a precondition (the zero row of owl_gemm_tn_slab_bf16, the zero pad columns of a transposed weight-gradient operand) unchanged.
Every comparison is exact: there is no tolerance in this file.  The last tests run the same question through the ops wrappers that cache their scratch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops, weights  # noqa: E402
from owl_vit_object_detection_amd import preprocess as PP  # noqa: E402
from owl_vit_object_detection_amd.matcher import PackedTargets  # noqa: E402
from tests import image_query_reference as IQ  # noqa: E402
from tests import open_vocab_loss_reference as OL  # noqa: E402
from tests import postprocess_reference as PR  # noqa: E402
from tests import slice_merge_reference as SM  # noqa: E402

DEV = "cuda"
TAIL = 4096          # guard bytes behind every scratch allocation
GUARD = 0xA5
NAN = float("nan")
bf = torch.bfloat16
STATES = ("zero", "ones", "after")


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------
class Case:
    """scratch: {name: bytes the entry's query (or its header) asks for}; run(scr) with scr = {name: uint8 view of exactly those bytes} makes fresh
    sentinel-filled outputs, calls the entry, synchronises and returns {name: output tensor}; guards: {name: tensor that must not change}."""

    def __init__(self, what, scratch, run, guards=None):
        self.what, self.scratch, self.run, self.guards = what, dict(scratch), run, dict(guards or {})


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


def _query(name, *args):
    n = torch.zeros(1, dtype=torch.int64)
    _lib.call(name, *args, n)
    return int(n.item())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=g)


def _sent(rows, width, dtype=torch.float32, extra=3):
    """[rows + extra, width] of a finite sentinel: the entry gets the base pointer, rows it does not own keep the value (and every run starts the same)."""
    return torch.full((rows + extra, width), 7 if dtype.is_floating_point else -7, dtype=dtype, device=DEV)


def _f32(scr):
    return scr.view(torch.float32)


def check_entry(probe, pred):
    assert set(probe.scratch) == set(pred.scratch), (probe.what, pred.what)
    bufs = {k: torch.empty(max(probe.scratch[k], pred.scratch[k]) + TAIL, dtype=torch.uint8, device=DEV) for k in probe.scratch}
    assert any(pred.scratch[k] > probe.scratch[k] for k in bufs) or all(probe.scratch[k] == pred.scratch[k] for k in bufs), "the predecessor is the larger problem"
    results = {}
    for state in STATES:
        for k, b in bufs.items():
            b.fill_(GUARD)
            if state != "after":
                b[:probe.scratch[k]] = 0x00 if state == "zero" else 0xFF
        if state == "after":
            pred.run({k: b[:pred.scratch[k]] for k, b in bufs.items()})
            torch.cuda.synchronize()
            for k, b in bufs.items():
                assert bool((b[pred.scratch[k]:] == GUARD).all()), f"{pred.what}: wrote behind its {k} ({pred.scratch[k]} bytes)"
            assert any(bool((b[:probe.scratch[k]] != 0).any()) for k, b in bufs.items()), f"{pred.what}: left the probe's scratch all zero: state `after` would be state `zero`"
        behind = {k: b[probe.scratch[k]:].clone() for k, b in bufs.items()}
        guards = {k: t.clone() for k, t in probe.guards.items()}
        out = probe.run({k: b[:probe.scratch[k]] for k, b in bufs.items()})
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert torch.equal(b[probe.scratch[k]:], behind[k]), f"{probe.what} ({state}): wrote behind its {k} ({probe.scratch[k]} bytes)"
        for k, t in probe.guards.items():
            assert torch.equal(_bits(t), _bits(guards[k])), f"{probe.what} ({state}): changed {k}, a buffer its callers rely on"
        results[state] = {k: v.detach().clone() for k, v in out.items()}
    base = results["zero"]
    for k, v in base.items():
        if v.dtype.is_floating_point:
            assert not bool(torch.isnan(v).any()), f"{probe.what}: NaN in {k} from finite inputs and zeroed scratch"
    for state in STATES[1:]:
        assert set(results[state]) == set(base)
        for k, v in results[state].items():
            if v.dtype.is_floating_point:
                assert not bool(torch.isnan(v).any()), f"{probe.what} (scratch: {state}): NaN in {k}"
            assert v.shape == base[k].shape and torch.equal(_bits(v), _bits(base[k])), f"{probe.what}: {k} depends on the scratch's earlier contents (zero vs {state})"


# ---- the row reductions (csrc/backward.hip: a partials kernel + partials_reduce_kernel) ---------------------------------------------------------
def ln_bwd(rows, D, dy_bf16, colsum, with_dx, seed=1):
    g = _gen(seed)
    x = _rn(g, rows, D)
    stats = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()], -1).contiguous().to(DEV)
    gamma = (1 + 0.1 * _rn(g, D)).to(DEV)
    dres = _rn(g, rows, D).to(DEV) if with_dx else None
    dy = _rn(g, rows, D).to(DEV)
    dy = dy.to(bf) if dy_bf16 else dy
    x = x.to(DEV)
    nbytes = _query("owl_rowreduce_workspace_bytes", 1, rows, D)

    def run(scr):
        dx, dxb = (_sent(rows, D), _sent(rows, D, bf)) if with_dx else (None, None)
        dg, db = torch.linspace(-1, 1, D, device=DEV), torch.linspace(2, -2, D, device=DEV)          # accumulated onto
        cs = torch.linspace(0.5, 1.5, D, device=DEV) if colsum else None
        part = _f32(scr["partials"])
        _lib.call("owl_layernorm_bwd", ops.stream(), dy, 1 if dy_bf16 else 0, x, stats, gamma, dres, dx, dg, db, rows, D, dxb, part, part.numel(), cs)
        torch.cuda.synchronize()
        out = dict(dgamma=dg, dbeta=db)
        if with_dx:
            out.update(dx=dx, dx_bf16=dxb)
        if colsum:
            out["dx_colsum"] = cs
        return out
    return Case(f"owl_layernorm_bwd rows={rows} D={D} dy={'bf16' if dy_bf16 else 'f32'} colsum={colsum} dx={with_dx}", dict(partials=nbytes), run)


def merge_bwd(B, P, Tp, D, seed=2):
    T, g = P + 1, _gen(seed)
    xv = _rn(g, B, T, D)
    g1, b1, g2 = 1 + 0.1 * _rn(g, D), 0.1 * _rn(g, D), 1 + 0.1 * _rn(g, D)
    m1, r1 = xv.mean(-1, keepdim=True), (xv.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    y1 = (xv - m1) * r1 * g1 + b1
    cls_ln = y1[:, 0].contiguous()
    merged = y1[:, 1:] * cls_ln[:, None]
    m2, r2 = merged.mean(-1, keepdim=True), (merged.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    x, st1 = torch.full((B * Tp, D), NAN), torch.full((B * Tp, 2), NAN)          # pad tokens: never read
    x.view(B, Tp, D)[:, :T] = xv
    st1.view(B, Tp, 2)[:, :T] = torch.cat([m1, r1], -1)
    st2 = torch.cat([m2, r2], -1).reshape(B * P, 2).contiguous()
    d = {k: v.to(DEV) for k, v in dict(x=x, st1=st1, st2=st2, cls_ln=cls_ln, g1=g1, b1=b1, g2=g2, dfeats=_rn(g, B * P, D)).items()}
    nbx = (P + 63) // 64

    def run(scr):
        dx, dxb = _sent(B * Tp, D), _sent(B * Tp, D, bf)
        acc = [torch.linspace(lo, hi, D, device=DEV) for lo, hi in ((-0.5, 0.75), (1.0, -0.25), (-1.5, -1.5), (0.25, 2.0), (2.0, 2.0))]
        part, dcls = _f32(scr["partials"]), _f32(scr["dcls_ws"])
        _lib.call("owl_merge_ln_bwd", ops.stream(), d["dfeats"], d["x"], d["cls_ln"], d["st1"], d["st2"], d["g1"], d["b1"], d["g2"], dx, dcls, acc[0], acc[1],
                  acc[2], acc[3], B, P, Tp, D, part, part.numel(), dxb, acc[4])
        torch.cuda.synchronize()
        return dict(dx=dx, dx_bf16=dxb, dcls=dcls.clone(), dg1=acc[0], db1=acc[1], dg2=acc[2], db2=acc[3], dx_colsum=acc[4])
    return Case(f"owl_merge_ln_bwd B={B} P={P} Tp={Tp} D={D}", dict(partials=4 * B * nbx * 6 * D, dcls_ws=4 * B * D), run)


def box_final_bwd(rows, D, seed=3):
    g = _gen(seed + rows)
    u1 = (1.5 * _rn(g, rows, D)).to(bf)
    h1 = torch.nn.functional.gelu(u1.float()).to(bf)
    d = {k: v.to(DEV) for k, v in dict(u1=u1, h1=h1, w2=0.1 * _rn(g, 4, D), sig=torch.sigmoid(_rn(g, rows, 4)), dboxes=_rn(g, rows, 4)).items()}
    nblk = _lib.load().owl_box_final_bwd_blocks(rows)

    def run(scr):
        du1 = _sent(rows, D, bf)
        gw, cs = torch.linspace(-1, 1, 4 * D + 4, device=DEV), torch.linspace(1, 2, D, device=DEV)
        _lib.call("owl_box_final_bwd", ops.stream(), d["dboxes"], d["sig"], d["h1"], d["u1"], d["w2"], du1, _f32(scr["partials"]), gw, rows, D, cs)
        torch.cuda.synchronize()
        return dict(du1=du1, dw2_db2=gw, du1_colsum=cs)
    return Case(f"owl_box_final_bwd rows={rows} D={D} ({nblk} blocks)", dict(partials=4 * nblk * (5 * D + 4)), run)


def colsum(kind, R, C, seed=4):
    g = _gen(seed + R)
    src = _rn(g, R, C).to(DEV)
    src = src if kind == "f32" else src.to(bf)
    nbytes = _query("owl_rowreduce_workspace_bytes", 1, R, C)
    ld = ops.pad_rows(R)
    out_t = torch.zeros(C, ld, dtype=bf, device=DEV) if kind == "transpose" else None          # as autograd._bws makes tA / tB: zeroed once, for good
    pad = {"out_t pad columns": out_t[:, R:]} if out_t is not None else {}

    def run(scr):
        cs = torch.linspace(-3, 3, C, device=DEV)
        part = _f32(scr["partials"])
        if kind == "f32":
            _lib.call("owl_colsum_f32", ops.stream(), src, cs, R, C, part, part.numel())
        elif kind == "bf16":
            _lib.call("owl_colsum_bf16", ops.stream(), src, C, cs, R, C, part, part.numel())
        else:
            _lib.call("owl_transpose_colsum_bf16", ops.stream(), src, C, out_t, ld, cs, R, C, part, part.numel())
        torch.cuda.synchronize()
        out = dict(colsum=cs)
        if out_t is not None:
            assert bool((out_t[:, R:].view(torch.int16) == 0).all()), "pad columns of the transposed operand"
            out["out_t"] = out_t.clone()
        return out
    name = {"f32": "owl_colsum_f32", "bf16": "owl_colsum_bf16", "transpose": "owl_transpose_colsum_bf16"}[kind]
    return Case(f"{name} R={R} C={C}", dict(partials=nbytes), run, guards=pad)


# ---- attention backward: dvec_ws -------------------------------------------------------------------------------------------------------------
def attn_bwd(B, H, T, seed=5):
    Tp, D = (T + 7) // 8 * 8, H * 64
    M, g = B * Tp, _gen(seed + T)
    qkv = torch.zeros(ops.pad_rows(M), 3 * D, dtype=bf, device=DEV)
    qkv[:M] = _rn(g, M, 3 * D).to(bf).to(DEV)
    O = torch.zeros(ops.pad_rows(M), D, dtype=bf, device=DEV)
    lse = torch.zeros(B, H, Tp, device=DEV)
    ops.attention_fwd_vrow(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, O, D, lse, B, H, T, Tp, 0.125)
    dO = torch.zeros(ops.pad_rows(M), D, dtype=bf, device=DEV)
    dO[:M] = (0.1 * _rn(g, M, D)).to(bf).to(DEV)
    dO[:M].view(B, Tp, D)[:, T:] = 0
    torch.cuda.synchronize()
    nbytes = _query("owl_attention_bwd_workspace_bytes", B, H, Tp)

    def run(scr):
        dqkv = torch.full((ops.pad_rows(M), 3 * D), 7.0, dtype=bf, device=DEV)
        _lib.call("owl_attention_bwd_bf16", ops.stream(), qkv, dO, O, lse, _f32(scr["dvec_ws"]), dqkv, B, H, T, Tp, 0.125, 0)
        torch.cuda.synchronize()
        assert bool((dqkv[M:] == 7.0).all()), "rows past B Tp written"
        return dict(dqkv=dqkv[:M].view(B, Tp, 3 * D)[:, :T].contiguous())
    return Case(f"owl_attention_bwd_bf16 (B, H, T)=({B}, {H}, {T})", dict(dvec_ws=nbytes), run)


# ---- open-vocabulary class head: rowstats (the forward's), the backward's workspace, rowgrad ---------------------------------------------------------
def class_logits(B, P, Q, Dt, D, want_dq, head, seed=6):
    g = _gen(seed + P)
    mask = torch.ones(B, Q, dtype=torch.uint8)
    mask[0, Q // 2] = 0
    mask[B - 1, Q - 1] = 0
    d = dict(e=_rn(g, B * P, Dt), queries=_rn(g, B, Q, Dt), feats=_rn(g, B * P, D).to(bf), w_shift=_rn(g, D, scale=0.3 / D ** 0.5),
             w_scale=_rn(g, D, scale=1 / D ** 0.5), b_shift=torch.tensor([0.05]), b_scale=torch.tensor([0.1]), mask=mask, dlogits=_rn(g, B, P, Q))
    d = {k: v.contiguous().to(DEV) for k, v in d.items()}
    scratch = dict(rowstats=8 * B * P)
    if head:
        scratch.update(workspace=ops.class_logits_bwd_head_workspace_bytes(B, P, Q, B, Dt, D, want_dq), rowgrad=8 * B * P)
    else:
        scratch.update(workspace=ops.class_logits_bwd_workspace_bytes(B, P, Q, B, Dt, want_dq))

    def run(scr):
        s, rowstats, ws = ops.stream(), _f32(scr["rowstats"]), scr["workspace"]
        logits, de, df = _sent(B * P, Q), _sent(B * P, Dt, bf), _sent(B * P, D)
        dq = _sent(B * Q, Dt) if want_dq else None
        _lib.call("owl_class_logits_fwd", s, d["e"], d["queries"], d["feats"], d["w_shift"], d["b_shift"], d["w_scale"], d["b_scale"], d["mask"], rowstats, logits,
                  None, B, P, Q, B, B, Dt, D)
        out = dict(logits=logits, de=de, dfeats=df)
        if head:
            dh, rowgrad = torch.full((2 * D + 2 + 3,), 7.0, device=DEV), _f32(scr["rowgrad"])
            _lib.call("owl_class_logits_bwd_head", s, d["dlogits"], d["e"], d["queries"], d["feats"], d["w_shift"], d["w_scale"], rowstats, d["mask"], ws, ws.numel(),
                      rowgrad, de, df, dq, dh[:D], dh[D:2 * D], dh[2 * D:2 * D + 1], dh[2 * D + 1:], B, P, Q, B, B, Dt, D)
            torch.cuda.synchronize()
            out.update(dhead=dh, rowgrad=rowgrad.clone())
        else:
            _lib.call("owl_class_logits_bwd", s, d["dlogits"], d["e"], d["queries"], d["w_shift"], d["w_scale"], rowstats, d["mask"], ws, ws.numel(), de, df, dq,
                      B, P, Q, B, B, Dt, D)
            torch.cuda.synchronize()
        out["rowstats"] = rowstats.clone()
        if want_dq:
            out["dqueries"] = dq
        return out
    return Case(f"owl_class_logits_fwd + owl_class_logits_bwd{'_head' if head else ''} (B, P, Q, Dt, D)=({B}, {P}, {Q}, {Dt}, {D}) dqueries={want_dq}", scratch, run)


# ---- image-guided query selection ------------------------------------------------------------------------------------------------------------
def image_query(N, P, Dt, seed):
    e, boxes, qbox = (t.to(DEV) for t in IQ.make_case("randn", N, P, Dt, seed=seed))

    def run(scr):
        best, info = _sent(N, 1, torch.int32, extra=1).view(-1), _sent(N, 2, torch.int32, extra=1)
        query, v = _sent(N, Dt, extra=1), _sent(N, P, extra=1)
        mean, sim = _sent(N, Dt, torch.float64, extra=1), _sent(N, P, torch.float64, extra=1)
        ws = scr["workspace"]
        _lib.call("owl_image_query_select", ops.stream(), e, boxes, qbox, N, P, Dt, ws, ws.numel(), best, query, info, v, mean, sim)
        torch.cuda.synchronize()
        return dict(best=best, info=info, query=query, v=v, mean=mean, sim=sim)
    return Case(f"owl_image_query_select (N, P, Dt)=({N}, {P}, {Dt})", dict(workspace=ops.image_query_workspace_bytes(N, P, Dt)), run)


# ---- sliced inference: the merge -------------------------------------------------------------------------------------------------------------
def _dense_ragged():
    """The `ragged` case's slices and xforms with every slot of every slice live: the same (G, Nmax), 350 candidates instead of 230."""
    c = SM.case("ragged")
    K, xf = c["K"], c["xform"]
    f0, s0, c0 = SM.random_candidates(K, 3, 111, True)
    f1, s1, c1 = SM.random_candidates(6 * K, 3, 112, True)
    return SM.pack(SM.spread(f0, s0, c0, xf[:1]) + SM.spread(f1, s1, c1, xf[1:]), xf, [0, 1, 7], 0.45, K=K)


def slice_merge(c, metric, what):
    G, N = len(c["slice_offsets"]) - 1, SM.n_max(c)
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(DEV) for k in ("boxes", "scores", "classes", "counts", "xform", "slice_offsets")}
    T, K = t["scores"].shape

    def run(scr):
        ob, os_ = _sent(G * N, 4), _sent(G * N, 1)
        oc, osrc, cnt = _sent(G * N, 1, torch.int64), _sent(G * N, 1, torch.int64), _sent(G, 1, torch.int32)
        ws = scr["workspace"]
        _lib.call("owl_slice_merge", ops.stream(), t["boxes"], t["scores"], t["classes"], t["counts"], t["xform"], t["slice_offsets"], ws, ws.numel(), ob, os_, oc,
                  osrc, cnt, T, K, G, N, N, float(c["thr"]), ops.MERGE_METRICS[metric], 1)
        torch.cuda.synchronize()
        return dict(boxes=ob, scores=os_, classes=oc, src=osrc, counts=cnt)
    return Case(f"owl_slice_merge {what} {metric} (G, Nmax)=({G}, {N})", dict(workspace=_query("owl_slice_merge_workspace", G, N)), run)


# ---- open-vocabulary criterion: owl_focal_loss_fwd + owl_box_pair_loss write the workspace, owl_open_vocab_loss_reduce reads it ------------------------
def ov_loss(name):
    case = OL.gpu_case(name)
    B, P, Q = case["logits"].shape
    lg, bx = case["logits"].to(DEV).contiguous(), case["boxes"].to(DEV).contiguous()
    mask = None if case["mask"] is None else case["mask"].to(DEV).to(torch.uint8).contiguous()
    nmasks = 1 if mask is None else int(mask.shape[0])
    tg = PackedTargets(case["labels"], case["tgt"], DEV, None, allow_empty=True)
    nb, N, s = float(max(1, sum(case["counts"]))), tg.Nmax, ops.stream()
    costT = torch.zeros(B, N, P, device=DEV)
    _lib.call("owl_focal_match_cost", s, lg, mask, bx, tg.labels, tg.boxes, tg.counts, costT, B, P, Q, nmasks, N, 0.25, 1.0, 5.0, 2.0)
    pred_idx, tgt_idx = torch.empty(B, N, dtype=torch.int64, device=DEV), torch.empty(B, N, dtype=torch.int64, device=DEV)
    tc = torch.empty(B, P, dtype=torch.int64, device=DEV)
    _lib.call("owl_hungarian", s, costT, tg.labels, tg.counts, pred_idx, tgt_idx, tc, B, P, N, Q)
    torch.cuda.synchronize()
    nbytes = _query("owl_focal_loss_workspace_bytes", B, P, Q)

    def run(scr):
        ws = scr["workspace"]
        dl1, dgiou, losses = _sent(B * P, 4), _sent(B * P, 4), torch.full((3 + 3,), 7.0, device=DEV)
        _lib.call("owl_focal_loss_fwd", s, lg, mask, tc, ws, nbytes, B, P, Q, nmasks, 0.25)
        _lib.call("owl_box_pair_loss", s, bx, mask, tg.labels, tg.boxes, pred_idx, tgt_idx, tg.counts, ws, nbytes, dl1, dgiou, B, P, Q, nmasks, N)
        _lib.call("owl_open_vocab_loss_reduce", s, ws, nbytes, losses, B, P, Q, nb)
        torch.cuda.synchronize()
        return dict(losses=losses, dl1=dl1, dgiou=dgiou)
    return Case(f"owl_focal_loss_fwd + owl_box_pair_loss + owl_open_vocab_loss_reduce `{name}` (B, P, Q)=({B}, {P}, {Q})", dict(workspace=nbytes), run)


# ---- the device input stage: tmp (the horizontal pass's intermediate) and the colour path's workspace ------------------------------------------------
def _sources(seed, shapes):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(DEV) for h, w in shapes]


def pre_batch(size, shapes, seed):
    ip = PP.DeviceImageProcessor(size, device=DEV)
    imgs = _sources(seed, shapes)
    rows, off, max_h = [], 0, 0
    for im in imgs:          # (DeviceImageProcessor.__call__'s descriptor, with the intermediate in this test's buffer)
        H, W = int(im.shape[0]), int(im.shape[1])
        bx, kx, ksx = ip._axis_tables(W, size)
        by, ky, ksy = ip._axis_tables(H, size)
        rows.append((im.data_ptr(), H, W, bx.data_ptr(), kx.data_ptr(), ksx, by.data_ptr(), ky.data_ptr(), ksy, off))
        off += (H * size * 3 + 255) // 256 * 256
        max_h = max(max_h, H)
    desc = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(DEV)

    def run(scr):
        out = torch.full((len(imgs) + 1, 3, size, size), 7.0, device=DEV)
        _lib.call("owl_preprocess_u8_batch", ops.stream(), desc, len(imgs), max_h, scr["tmp"], ip.lut, out, 0, size, size)
        torch.cuda.synchronize()
        return dict(out=out)
    return Case(f"owl_preprocess_u8_batch {len(imgs)} images -> {size}", dict(tmp=off), run, guards={f"source {i}": im for i, im in enumerate(imgs)})


def pre_tiles(size, grid, n_out, shapes, seed, color):
    ip = PP.DeviceImageProcessor(size, device=DEV)
    imgs = _sources(seed, shapes)
    rs = np.random.RandomState(seed + 1)
    cell, tiles = size // grid, []
    for b in range(n_out):
        for j in range(grid * grid):
            src = int(rs.randint(len(imgs)))
            H, W = shapes[src]
            l, u = rs.uniform(0, W * 0.3), rs.uniform(0, H * 0.3)
            tiles.append(PP.Tile(src, (l, u, l + W * 0.6, u + H * 0.6), bool(j & 1), b, (j % grid) * cell, (j // grid) * cell, cell, cell))
    PP.check_tile_cover(tiles, n_out, size, shapes)
    desc, arena, tmp_bytes, max_rows = PP.build_tile_tables(shapes, tiles)
    arena_d = torch.from_numpy(arena).to(DEV)
    PP.resolve_tile_descs(desc, [im.data_ptr() for im in imgs], arena_d.data_ptr())
    desc_d = torch.from_numpy(desc).to(DEV)
    scratch = dict(tmp=tmp_bytes)
    color_d = None
    if color:
        rows = np.column_stack([rs.uniform(0.4, 1.6, (len(tiles), 3)), rs.randint(0, 6, len(tiles))])
        color_d = torch.from_numpy(PP.check_color(rows, len(tiles))).to(DEV)
        scratch["workspace"] = PP.color_workspace_bytes(len(tiles), size)

    def run(scr):
        out = torch.full((n_out + 1, 3, size, size), 7.0, device=DEV)
        if color:
            ws = scr["workspace"]
            _lib.call("owl_preprocess_u8_tiles_color", ops.stream(), desc_d, color_d, len(tiles), max_rows, scr["tmp"], ws, ws.numel(), ip.lut, out, 0, n_out, size, size)
        else:
            _lib.call("owl_preprocess_u8_tiles", ops.stream(), desc_d, len(tiles), max_rows, scr["tmp"], ip.lut, out, 0, n_out, size, size)
        torch.cuda.synchronize()
        assert bool((out[n_out] == 7.0).all()), "an image past n_out written"
        return dict(out=out)
    return Case(f"owl_preprocess_u8_tiles{'_color' if color else ''} {len(tiles)} tiles -> {n_out} x {size}", scratch, run,
                guards=dict({"arena": arena_d, "desc": desc_d}, **{f"source {i}": im for i, im in enumerate(imgs)}))          # (held here: the descriptors carry raw addresses)


# ---- the box head's row path: row_list / count_flag are state the three other kernels read ---------------------------------------------------------
def box_rows(rows, D, cap, listed, seed=8):
    g = _gen(seed + rows)
    db = torch.zeros(rows, 4)
    db[torch.as_tensor(listed, dtype=torch.int64)] = _rn(g, len(listed), 4)
    db = db.to(DEV)
    src = [_rn(g, rows, D).to(bf).to(DEV) for _ in range(3)]
    cap_pad = ops.box_rows_cap_pad(cap)
    comp = _rn(g, cap_pad, D).to(bf).to(DEV)
    dfc, base = _rn(g, cap_pad, D).to(DEV), _rn(g, rows, D).to(DEV)
    want, over = sorted(listed)[:cap], len(listed) > cap

    def run(scr):
        rl, cf, s = scr["row_list"].view(torch.int32), scr["count_flag"].view(torch.int32), ops.stream()
        _lib.call("owl_box_rows_compact", s, db, rows, cap, rl, cf)
        torch.cuda.synchronize()
        assert cf[:2].tolist() == [len(want), int(over)] and rl[:len(want)].tolist() == want, (cf[:2].tolist(), rl.tolist(), want)          # its OWN count, its own flag
        out = dict(count_flag=cf[:2].clone(), row_list=rl[:len(want)].clone())
        if over:          # (the predecessor: what it leaves behind is its row list and the set overflow flag; the other three kernels keep no state)
            return out
        dst = [_sent(cap_pad, D, bf) for _ in range(3)]
        _lib.call("owl_box_rows_gather", s, src[0], src[1], src[2], dst[0], dst[1], dst[2], rl, cf, rows, cap_pad, D)
        put = [torch.zeros(rows + 3, D, dtype=bf, device=DEV) for _ in range(2)]
        _lib.call("owl_box_rows_put", s, comp, None, put[0], put[1], rl, cf, rows, cap, D)
        acc = torch.cat([base, torch.full((3, D), 7.0, device=DEV)])
        _lib.call("owl_box_rows_scatter_add", s, dfc, acc, rl, cf, rows, cap, D)
        torch.cuda.synchronize()
        keep = torch.ones(rows + 3, dtype=torch.bool, device=DEV)
        keep[torch.as_tensor(want, dtype=torch.int64, device=DEV)] = False
        assert bool((put[0][keep].view(torch.int16) == 0).all()) and bool((put[1].view(torch.int16) == 0).all()), "put wrote a row that is not listed"
        assert torch.equal(acc[keep][:-3], base[keep[:-3]]), "scatter_add touched a row that is not listed"
        out.update(gather0=dst[0], gather1=dst[1], gather2=dst[2], put0=put[0], put1=put[1], scatter=acc)
        return out
    return Case(f"owl_box_rows_compact / gather / put / scatter_add rows={rows} D={D} cap={cap} listed={len(listed)}",
                dict(row_list=4 * cap, count_flag=4 * ops.box_rows_state_ints(rows)), run)


# ---- other entries the header gives a scratch pointer -------------------------------------------------------------------------------------------
def tn_slab(M, N, K, splits, seed=9):
    """owl_gemm_tn_slab_bf16 (slab, bias_slab; zero_row is a precondition) + owl_slab_reduce, which reads splits_used slabs."""
    g = _gen(seed + M)
    dy = torch.full((ops.pad_rows(M), N), 7.0, dtype=bf, device=DEV)
    x = torch.full((ops.pad_rows(M), K), 3.0, dtype=bf, device=DEV)          # pad rows must not leak into the sum
    dy[:M], x[:M] = (0.1 * _rn(g, M, N)).to(bf).to(DEV), _rn(g, M, K).to(bf).to(DEV)
    zero_row = torch.zeros(512, dtype=bf, device=DEV)
    nbytes = _query("owl_gemm_tn_slab_workspace_bytes", M, N, K, splits)

    def run(scr):
        used = torch.zeros(1, dtype=torch.int32)
        slab, bslab, s = _f32(scr["slab"]), _f32(scr["bias_slab"]), ops.stream()
        _lib.call("owl_gemm_tn_slab_bf16", s, dy, N, x, K, zero_row, slab, M, N, K, splits, used, 0, bslab)
        ns = int(used.item())
        assert 1 <= ns <= splits and 4 * ns * N * K <= nbytes
        dw, dbias = torch.full((N * K + 8,), 7.0, device=DEV), torch.linspace(-1, 1, N, device=DEV)
        _lib.call("owl_slab_reduce", s, slab, dw, N * K, N * K, ns, 0)
        _lib.call("owl_slab_reduce", s, bslab, dbias, N, N, ns, 1)
        torch.cuda.synchronize()
        return dict(dw=dw, db=dbias, splits_used=torch.tensor([ns]))
    return Case(f"owl_gemm_tn_slab_bf16 + owl_slab_reduce (M, N, K)=({M}, {N}, {K}) splits={splits}", dict(slab=nbytes, bias_slab=4 * splits * N), run,
                guards={"zero_row": zero_row})


def nt_slab(M, N, K, splits, seed=10):
    """owl_gemm_nt_bf16 epilogue 11 (split-K slabs) + owl_slab_reduce over owl_gemm_effective_splits slabs."""
    g = _gen(seed + M)
    A, W = ops.zeros_rows(M, K, bf, DEV), ops.zeros_rows(N, K, bf, DEV)
    A[:M], W[:N] = _rn(g, M, K).to(bf).to(DEV), (0.1 * _rn(g, N, K)).to(bf).to(DEV)
    nbytes = _query("owl_gemm_slab_workspace_bytes", M, N, K, splits)
    ns = _lib.load().owl_gemm_effective_splits(K, splits)

    def run(scr):
        slab, out = _f32(scr["slab"]), torch.full((M * N + 8,), 7.0, device=DEV)
        _lib.call("owl_gemm_nt_bf16", ops.stream(), ops.EPI_SLAB_F32, A, K, A.shape[0], W, K, W.shape[0], None, slab, N, None, None, 0, M, N, K, 1.0, splits, 0, 0)
        _lib.call("owl_slab_reduce", ops.stream(), slab, out, M * N, M * N, ns, 0)
        torch.cuda.synchronize()
        return dict(out=out)
    return Case(f"owl_gemm_nt_bf16 epi 11 + owl_slab_reduce (M, N, K)=({M}, {N}, {K}) splits={splits} ({ns} used)", dict(slab=nbytes), run)


def nt_slab_rows(M, n_in, K, splits, seed=13):
    """The NT weight-gradient route of an inner size that is no multiple of 8 (autograd.weight_grad): epilogue-11 slabs [splits][M][Kp] with Kp = n_in rounded
    up to 8, the W operand's rows [n_in, Kp) absent (w_rows clamps the loads), then owl_slab_reduce_rows, which reads columns [0, n_in) of every slab row."""
    Kp, g = (n_in + 7) // 8 * 8, _gen(seed + M)
    assert Kp > n_in and n_in % 4 == 0
    A, W = ops.zeros_rows(M, K, bf, DEV), torch.full((ops.pad_rows(n_in), K), NAN, dtype=bf, device=DEV)          # rows past w_rows: never loaded
    A[:M], W[:n_in] = _rn(g, M, K).to(bf).to(DEV), (0.1 * _rn(g, n_in, K)).to(bf).to(DEV)
    nbytes = _query("owl_gemm_slab_workspace_bytes", M, Kp, K, splits)
    ns = _lib.load().owl_gemm_effective_splits(K, splits)

    def run(scr):
        slab, out = _f32(scr["slab"]), torch.linspace(-1, 1, M * n_in + 8, device=DEV)          # accumulated onto; the last 8 are not the entry's
        tail = out[M * n_in:].clone()
        _lib.call("owl_gemm_nt_bf16", ops.stream(), ops.EPI_SLAB_F32, A, K, A.shape[0], W, K, n_in, None, slab, Kp, None, None, 0, M, Kp, K, 1.0, splits, 0, 0)
        _lib.call("owl_slab_reduce_rows", ops.stream(), slab, out, M, n_in, Kp, M * Kp, ns, 1)
        torch.cuda.synchronize()
        assert torch.equal(out[M * n_in:], tail), "owl_slab_reduce_rows wrote past [rows, cols]"
        return dict(out=out)
    return Case(f"owl_gemm_nt_bf16 epi 11 + owl_slab_reduce_rows (M, n_in, Kp, K)=({M}, {n_in}, {Kp}, {K}) splits={splits} ({ns} used)", dict(slab=nbytes), run)


def grad_norm(n, seed=11, ema=False):
    """owl_grad_sumsq writes one f64 per workgroup; the clipped step adds them in its own prologue: owl_adamw_step_grouped (csrc/optim_groups.hip) or, ema=True,
    owl_adamw_step_ema (csrc/optim_ema.hip: its own kernel and its own copy of that prologue; what FusedAdamW(ema_decay=) launches)."""
    g = _gen(seed + n)
    grad, p0 = _rn(g, n).to(DEV), _rn(g, n).to(DEV)
    seg = torch.tensor([n], dtype=torch.int64)
    nbytes = _query("owl_grad_norm_workspace_bytes", n)

    def run(scr):
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        pb, norm = torch.full((n + 8,), 7.0, dtype=bf, device=DEV), torch.full((4,), 7.0, device=DEV)
        args = (ops.stream(), p, grad, m, v, pb, n, 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, 1.0, seg, None, None, 1, 0.05, scr["workspace"], norm)
        _lib.call("owl_grad_sumsq", ops.stream(), grad, n, scr["workspace"])
        out = dict(p=p, m=m, v=v, p_bf16=pb, norm=norm)
        if ema:
            out["ema"] = torch.cat([p0, torch.full((8,), 7.0, device=DEV)])
            _lib.call("owl_adamw_step_ema", *args, out["ema"], 0.99, 0.01)
        else:
            _lib.call("owl_adamw_step_grouped", *args)
        torch.cuda.synchronize()
        return out
    return Case(f"owl_grad_sumsq + owl_adamw_step_{'ema' if ema else 'grouped'} n={n}", dict(workspace=nbytes), run)


def push_pull(B, P, C, counts, seed=14):
    """owl_push_pull_loss: per_image f32 [B, 4] is written by the class and the box kernel and added up by the third."""
    from owl_vit_object_detection_amd.losses import PushPullLoss
    g, rs = _gen(seed + P), np.random.RandomState(seed + P)
    sims = _rn(g, B, P, C, scale=0.3).to(DEV)
    c, wh = torch.rand(B, P, 2, generator=g) * 0.6 + 0.2, torch.rand(B, P, 2, generator=g) * 0.3 + 0.05
    boxes = torch.cat([c - wh / 2, c + wh / 2], -1).contiguous().to(DEV)
    labels = [torch.from_numpy(rs.randint(0, C, n).astype(np.int64)).to(DEV) for n in counts]
    tgt = []
    for n in counts:
        xy, w = rs.rand(n, 2) * 0.6, 0.02 + rs.rand(n, 2) * 0.35
        tgt.append(torch.from_numpy(np.concatenate([xy, xy + w], 1).astype(np.float32)).to(DEV))
    crit = PushPullLoss(C, None)
    tg = PackedTargets(labels, tgt, DEV, crit.background_label)
    tc, pred_idx, tgt_idx, _ = crit.matcher.match_packed(sims, boxes, tg)
    _lib.call("owl_spread_labels", ops.stream(), boxes, tc, B, P, crit.background_label, 0.85)
    torch.cuda.synchronize()

    def run(scr):
        per_image = _f32(scr["per_image"])
        lo, dsims, dl1, dgiou = torch.full((4 + 4,), 7.0, device=DEV), _sent(B * P, C), _sent(B * P, 4), _sent(B * P, 4)
        _lib.call("owl_push_pull_loss", ops.stream(), sims, boxes, tc, None, tg.boxes, pred_idx, tgt_idx, tg.counts, per_image, lo, dsims, dl1, dgiou,
                  B, P, C, tg.Nmax, crit.background_label)
        torch.cuda.synchronize()
        return dict(losses=lo, dsims=dsims, dl1=dl1, dgiou=dgiou, per_image=per_image.clone())
    return Case(f"owl_push_pull_loss (B, P, C)=({B}, {P}, {C})", dict(per_image=16 * B), run)


def patch_embed(B, G, ps, D, seed=12, Gw=None):
    """The single-phase kernels' explicit im2row of a patch size that is not 2^n (tile 128).  Gw: a rectangular grid G x Gw through the _hw entries."""
    hw = Gw is not None
    Gw = Gw if hw else G
    S, P = G * ps, G * Gw
    Tp, g = (P + 1 + 7) // 8 * 8, _gen(seed + G)
    img = _rn(g, B, 3, S, Gw * ps).to(bf).to(DEV)
    wk = weights.patch_weight_gather_layout(_rn(g, D, 3 * ps * ps, scale=0.05), ps).contiguous().to(bf).to(DEV)
    pos = _rn(g, P + 1, D).to(DEV)
    size = (S, Gw * ps) if hw else (S,)
    nbytes = _query("owl_patch_embed_scratch_bytes" + ("_hw" if hw else ""), B, *size, ps, D, 128)
    assert nbytes > 0

    def run(scr):
        x = _sent(B * Tp, D, extra=Tp)
        _lib.call("owl_patch_embed_bf16" + ("_hw" if hw else ""), ops.stream(), img, wk, pos, x, scr["scratch"], B, *size, ps, D, Tp, 128)
        torch.cuda.synchronize()
        return dict(x=x)
    return Case(f"owl_patch_embed_bf16{'_hw' if hw else ''} B={B} grid={G} x {Gw} ps={ps} D={D} tile 128", dict(scratch=nbytes), run)


# ---- the table: name -> (probe, the larger predecessor), both built on the device when the test runs -----------------------------------------------
ENTRIES = {}
# owl_layernorm_bwd: 130 rows = 3 partial blocks, the last of 2 rows; D = 128 the any-D body, 768 ln_bwd_kernel_768; predecessor 8 blocks at D = 1024
for _D in (128, 768):
    for _bf16, _cs, _dx in ((True, True, True), (True, False, True), (True, False, False), (False, False, True), (False, False, False)):
        ENTRIES[f"layernorm_bwd-D{_D}-{'bf16' if _bf16 else 'f32'}{'-colsum' if _cs else ''}{'' if _dx else '-nodx'}"] = (
            lambda D=_D, b=_bf16, c=_cs, x=_dx: ln_bwd(130, D, b, c, x), lambda b=_bf16, c=_cs, x=_dx: ln_bwd(450, 1024, b, c, x, seed=21))
ENTRIES["layernorm_bwd-D1024-bf16-colsum"] = (lambda: ln_bwd(130, 1024, True, True, True), lambda: ln_bwd(450, 1024, True, True, True, seed=21))          # the third instantiation
ENTRIES["merge_ln_bwd"] = (lambda: merge_bwd(2, 70, 72, 128), lambda: merge_bwd(3, 200, 208, 256, seed=22))
ENTRIES["merge_ln_bwd-D768"] = (lambda: merge_bwd(2, 70, 72, 768), lambda: merge_bwd(3, 200, 208, 1024, seed=22))
ENTRIES["box_final_bwd"] = (lambda: box_final_bwd(577, 64), lambda: box_final_bwd(2500, 64, seed=23))
ENTRIES["box_final_bwd-D768"] = (lambda: box_final_bwd(577, 768), lambda: box_final_bwd(2500, 768, seed=23))
for _kind in ("f32", "bf16", "transpose"):
    for _R in (130, 1000):
        ENTRIES[f"colsum_{_kind}-R{_R}"] = (lambda k=_kind, R=_R: colsum(k, R, 128), lambda k=_kind: colsum(k, 2100, 256, seed=24))
ENTRIES["attention_bwd"] = (lambda: attn_bwd(1, 2, 65), lambda: attn_bwd(2, 3, 193, seed=25))
for _head in (False, True):
    for _dq in (True, False):
        # 300 rows: two 256-row chunks of the head-gradient pass and several slabs of the dq^ partial sums; the predecessor has more of both, and wider rows
        ENTRIES[f"class_logits_bwd{'_head' if _head else ''}-{'dq' if _dq else 'nodq'}"] = (
            lambda h=_head, q=_dq: class_logits(2, 300, 5, 64, 128, q, h), lambda h=_head, q=_dq: class_logits(3, 600, 40, 128, 256, q, h, seed=26))
ENTRIES["image_query_select"] = (lambda: image_query(3, 36, 64, 5), lambda: image_query(3, 130, 64, 6))
for _metric in SM.METRICS:
    ENTRIES[f"slice_merge-{_metric}"] = (lambda m=_metric: slice_merge(SM.case("ragged"), m, "ragged"), lambda m=_metric: slice_merge(_dense_ragged(), m, "dense ragged"))
ENTRIES["open_vocab_loss"] = (lambda: ov_loss("q31_empty"), lambda: ov_loss("q70_tiny"))
ENTRIES["preprocess_u8_batch"] = (lambda: pre_batch(32, [(40, 52), (33, 47)], 31), lambda: pre_batch(48, [(90, 70), (64, 101), (77, 58)], 32))
ENTRIES["preprocess_u8_tiles"] = (lambda: pre_tiles(32, 2, 1, [(40, 52), (33, 47)], 33, False), lambda: pre_tiles(48, 3, 2, [(90, 70), (64, 101), (77, 58)], 34, False))
ENTRIES["preprocess_u8_tiles_color"] = (lambda: pre_tiles(32, 2, 1, [(40, 52), (33, 47)], 35, True), lambda: pre_tiles(48, 3, 2, [(90, 70), (64, 101), (77, 58)], 36, True))
# the row list and (count, overflow flag) of an OVERFLOWING call on more rows (three compaction workgroups), then a call that lists three rows
ENTRIES["box_rows"] = (lambda: box_rows(577, 64, 8, [8, 300, 576]), lambda: box_rows(2500, 64, 8, [3, 100, 1023, 1024, 1500, 2047, 2048, 2300, 2499], seed=27))
ENTRIES["gemm_tn_slab"] = (lambda: tn_slab(300, 256, 256, 3), lambda: tn_slab(1000, 512, 256, 4, seed=28))
ENTRIES["gemm_nt_slab"] = (lambda: nt_slab(40, 136, 384, 3), lambda: nt_slab(300, 256, 1024, 8, seed=29))
ENTRIES["gemm_nt_slab_reduce_rows"] = (lambda: nt_slab_rows(40, 20, 384, 3), lambda: nt_slab_rows(136, 588, 1024, 8, seed=32))          # (588 -> 592: L/14's patch columns)
ENTRIES["grad_norm_adamw"] = (lambda: grad_norm(40004), lambda: grad_norm(400000, seed=30))
ENTRIES["grad_norm_adamw_ema"] = (lambda: grad_norm(40004, ema=True), lambda: grad_norm(400000, seed=30, ema=True))
ENTRIES["push_pull_loss"] = (lambda: push_pull(2, 36, 4, (2, 1)), lambda: push_pull(5, 144, 10, (3, 1, 6, 2, 4), seed=33))
ENTRIES["patch_embed_im2row"] = (lambda: patch_embed(2, 3, 10, 128), lambda: patch_embed(6, 5, 10, 128, seed=31))
ENTRIES["patch_embed_im2row_hw"] = (lambda: patch_embed(2, 3, 10, 128, Gw=4), lambda: patch_embed(6, 5, 10, 128, seed=31, Gw=6))


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_does_not_read_what_an_earlier_call_left(name):
    probe, pred = ENTRIES[name]
    check_entry(probe(), pred())


# ---- control: the harness fails on the mistakes it is there for (plain torch stand-ins for a kernel pair, no product code) --------------------------------
def _planted(mistake, blocks, seed):
    """A producer that writes `blocks` rows of 64 partial sums into scratch sized for blocks + 1, and a reducer that adds them.  Mistakes: the reducer adds
    one block more than was written; the producer writes one float behind the scratch; the pair increments a buffer its caller relies on."""
    x = _rn(_gen(seed), blocks, 64).to(DEV)
    guard = torch.zeros(4, device=DEV)
    nbytes = 4 * (blocks + 1) * 64

    def run(scr):
        part = _f32(scr["partials"])
        part[:blocks * 64] = x.view(-1)
        if mistake == "writes_behind":
            torch.as_strided(scr["partials"], (4,), (1,), nbytes).fill_(0)
        if mistake == "changes_a_guard":
            guard.add_(1.0)
        n = blocks + (1 if mistake == "one_block_more" else 0)
        out = part[:n * 64].view(n, 64).sum(0)
        torch.cuda.synchronize()
        return dict(colsum=out)
    return Case(f"planted {mistake}", dict(partials=nbytes), run, guards={"guard": guard})


@pytest.mark.parametrize("mistake,message", [("one_block_more", "NaN in colsum|depends on the scratch"), ("writes_behind", "wrote behind its partials"),
                                             ("changes_a_guard", "changed guard")])
def test_the_harness_fails_on_a_planted_mistake(mistake, message):
    check_entry(_planted(None, 3, 60), _planted(None, 7, 61))          # the same pair without a mistake passes
    with pytest.raises(AssertionError, match=message):
        check_entry(_planted(mistake, 3, 60), _planted(mistake, 7, 61))


# ---- the ops wrappers that keep their scratch between calls ---------------------------------------------------------------------------------------
def _same(a, b):
    return all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_postprocess_wrapper_after_a_denser_case_under_the_same_key():
    P = 200
    X = PR.cached_reference("random", P, 3, 2065, 65, PR.TEMPLATE_THR, PR.BASIC)[0]
    Y = PR.cached_reference("random", P, 3, 2200, 200, PR.TEMPLATE_THR, PR.BASIC)[0]

    def run(c, route):
        out = ops.postprocess(torch.from_numpy(c["boxes"]).to(DEV)[None], torch.from_numpy(c["sims"]).to(DEV)[None], P, float(c["conf"]), float(c["thr"]), route)
        torch.cuda.synchronize()
        return out
    for route in PR.BASIC:
        ops._pp_ws.clear()
        first = run(X, route)
        assert int(first[4][0]) > 0
        dense = run(Y, route)
        assert int(dense[4][0]) > int(first[4][0]) and len(ops._pp_ws) == 1          # the same cache key: the same workspace
        assert _same(run(X, route), first), route


def test_slice_merge_wrapper_after_a_denser_case_under_the_same_key():
    def run(c, metric):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        out = ops.slice_merge(t(c["boxes"]), t(c["scores"]), t(c["classes"]), t(c["counts"]), t(c["xform"]), t(c["slice_offsets"]), 2, SM.n_max(c), SM.n_max(c),
                              float(c["thr"]), metric, True)
        torch.cuda.synchronize()
        return out
    X, Y = SM.case("ragged"), _dense_ragged()
    assert SM.n_max(X) == SM.n_max(Y) and int(Y["counts"].sum()) > int(X["counts"].sum())          # the same key, more candidates
    for metric in SM.METRICS:
        ops._sm_ws.clear()
        first = run(X, metric)
        run(Y, metric)
        assert len(ops._sm_ws) == 1
        assert _same(run(X, metric), first), metric


def test_stand_alone_partials_buffer_after_wider_and_taller_reductions():
    """ops._part: one cached buffer per device serves every stand-alone row reduction, whatever its width and block count."""
    g = _gen(40)

    def probe():
        out = []
        for R, C in ((130, 128), (1000, 128)):
            src = _rn(_gen(41 + R), R, C).to(DEV)
            for kind in ("f32", "bf16", "transpose"):
                cs = torch.linspace(-3, 3, C, device=DEV)
                if kind == "f32":
                    ops.colsum_f32(src, cs, R, C)
                elif kind == "bf16":
                    ops.colsum_bf16(src.to(bf), cs, R, C)
                else:
                    ops.transpose_colsum(src.to(bf), None, cs, R, C)
                out.append(cs)
        torch.cuda.synchronize()
        return out

    def ln_through_wrapper(rows, D, seed):
        gg = _gen(seed)
        x = _rn(gg, rows, D)
        stats = torch.stack([x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()], -1).contiguous().to(DEV)
        dy, dres, gamma = _rn(gg, rows, D).to(bf).to(DEV), _rn(gg, rows, D).to(DEV), (1 + 0.1 * _rn(gg, D)).to(DEV)
        dx, dxb = torch.zeros(rows, D, device=DEV), torch.zeros(rows, D, dtype=bf, device=DEV)
        dg, db, cs = torch.ones(D, device=DEV), torch.ones(D, device=DEV), torch.ones(D, device=DEV)
        ops.layernorm_bwd(dy, x.to(DEV), stats, gamma, dres, dx, dg, db, rows, D, dx_bf16=dxb, dx_colsum=cs)
        torch.cuda.synchronize()
        return [dx, dxb, dg, db, cs]

    ops._partials.clear()
    first = probe() + ln_through_wrapper(130, 128, 50)
    # a taller and wider predecessor of every kind: the buffer grows, then holds their partial sums
    ln_through_wrapper(450, 1024, 51)
    big = _rn(g, 2100, 256).to(DEV)
    ops.colsum_f32(big, torch.zeros(256, device=DEV), 2100, 256)
    ops.colsum_bf16(big.to(bf), torch.zeros(256, device=DEV), 2100, 256)
    ops.transpose_colsum(big.to(bf), None, torch.zeros(256, device=DEV), 2100, 256)
    torch.cuda.synchronize()
    assert len(ops._partials) == 1
    assert _same(probe() + ln_through_wrapper(130, 128, 50), first)
