"""What training HF's logit shift and scale costs on the card: `owl_class_logits_bwd_head` beside `owl_class_logits_bwd` at B/16 768^2 batch 32
(rows = 32 x 2304, Dt = 512, D = 768) for Q = 30, 91 and 365 queries per image, per-image banks and masks, no query gradient; the torch-ops product
`rowgrad.T @ feats.float()` that gives the same two weight gradients; and the whole `forward_queries` + `OpenVocabLoss` train step on
owlvit-base-patch16, batch 32, 91 queries, with the head frozen (the launches of a build without this feature) and trained.
  python tools/logit_head_grad_timing.py [--out profiles/logit_head_train.md] [--windows 5] [--launches 10] [--limit 600] [--no-model] [--no-trace]
Method.  Calls: one fresh child process under its own time limit; a window is `--launches` launches (3 steps for the whole-model rows) between two HIP
events, the forms alternate window by window after a warm-up window of each; every figure is the median of `--windows` windows (min .. max).
Kernels: the two entries differ by two launches and one store inside a kernel both share, which no event can separate -- a SECOND child runs the two
entries under `rocprofv3 --kernel-trace` (a run of its own: tracing slows the host, no call time is taken from it) and the per-kernel times are read
from the trace, told apart by the order the child launched them in (a row pass that the partial-sum launch follows stored its scalars).  Bytes of the
reduction: the algorithm's -- rows x D bf16 features and rows x 2 f32 row scalars read once -- over the partial-sum kernel's time.
Recorded, not asserted."""
import argparse, csv, glob, json, os, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

B, P, DT, D = 32, 2304, 512, 768
QS = (30, 91, 365)
STEP_Q = 91
NT = 5                      # targets per image of the train-step rows
LN_STREAM_TBS = 6.2          # what the LayerNorm kernels stream at (profiles/): the yardstick for a pass bound by one read


def kernel_operands(torch, ops, Q, g, dev):
    rows = B * P
    e = (0.7 * torch.randn(rows, DT, generator=g)).to(dev)
    feats = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(dev)
    w_shift, w_scale = (torch.randn(D, generator=g) / D ** 0.5).to(dev), (torch.randn(D, generator=g) / D ** 0.5).to(dev)
    b_shift, b_scale = torch.tensor([0.05], device=dev), torch.tensor([0.1], device=dev)
    rowstats = torch.empty(rows, 2, device=dev)
    bank = torch.randn(B, Q, DT, generator=g).to(dev)
    mask = (torch.rand(B, Q, generator=g) > 0.1).to(torch.uint8).to(dev)
    ops.class_logits(e, bank, feats, w_shift, b_shift, w_scale, b_scale, B, P, mask=mask, rowstats=rowstats)
    dlog = torch.empty(B, P, Q, device=dev).normal_().mul_(0.1)
    de, dfeats = torch.empty(rows, DT, dtype=torch.bfloat16, device=dev), torch.empty(rows, D, device=dev)
    rowgrad, dhead = torch.empty(rows, 2, device=dev), torch.empty(2 * D + 2, device=dev)
    wsp = torch.empty(ops.class_logits_bwd_head_workspace_bytes(B, P, Q, B, DT, D, False), dtype=torch.uint8, device=dev)
    common = dict(mask=mask, de=de, dfeats=dfeats, dqueries=False, workspace=wsp)
    frozen = lambda: ops.class_logits_bwd(dlog, e, bank, w_shift, w_scale, rowstats, B, P, **common)
    trained = lambda: ops.class_logits_bwd(dlog, e, bank, w_shift, w_scale, rowstats, B, P, feats=feats, dhead=dhead, rowgrad=rowgrad, **common)
    return frozen, trained, rowgrad, feats


def child_trace(launches):
    """Under rocprofv3: per Q, two warm-up calls of each entry, then `launches` calls of the one and `launches` of the other; the parent tells them
    apart by the order of the dispatches (read_trace)."""
    import torch
    from owl_vit_object_detection_amd import ops
    g = torch.Generator().manual_seed(0)
    for Q in QS:
        frozen, trained, _, _ = kernel_operands(torch, ops, Q, g, "cuda")
        for fn in (frozen, trained, frozen, trained):
            fn()
        torch.cuda.synchronize()
        for fn in (frozen, trained):
            for _ in range(launches):
                fn()
            torch.cuda.synchronize()
    print("TRACED", flush=True)


def child(windows, launches, with_model):
    import torch
    from owl_vit_object_detection_amd import ops
    dev = "cuda"

    def between_events(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3          # us

    def measure(forms, n):
        for fn in forms.values():
            between_events(fn, 2)
        us = {k: [] for k in forms}
        for _ in range(windows):
            for k, fn in forms.items():
                us[k].append(between_events(fn, n))
        return {k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in us.items()}

    g = torch.Generator().manual_seed(0)
    out = []
    for Q in QS:
        frozen, trained, rowgrad, feats = kernel_operands(torch, ops, Q, g, dev)
        trained()
        forms = dict(frozen=frozen, trained=trained, torch_product=lambda: rowgrad.t() @ feats.float())
        out.append(dict(Q=Q, us=measure(forms, launches)))
        del frozen, trained, rowgrad, feats, forms
        torch.cuda.empty_cache()
    model_res = None
    if with_model:
        from owl_vit_object_detection_amd import synth, weights
        from owl_vit_object_detection_amd.config import get_config
        from owl_vit_object_detection_amd.losses import OpenVocabLoss
        from owl_vit_object_detection_amd.models import OwlViT
        from owl_vit_object_detection_amd.optim import FusedAdamW
        cfg = get_config("owlvit-base-patch16")
        model = OwlViT(cfg, weights.make_weights(cfg), dev)
        head = {"logit_shift.weight": torch.randn(D, generator=g) / D ** 0.5, "logit_shift.bias": torch.tensor([0.05]),
                "logit_scale.weight": torch.randn(D, generator=g) / D ** 0.5, "logit_scale.bias": torch.tensor([0.1])}
        opt = FusedAdamW(model, lr=1e-5, weight_decay=0.1)
        img = torch.from_numpy(synth.make_images(cfg, 4)).to(dev).repeat(B // 4, 1, 1, 1).to(torch.bfloat16)
        qe = torch.randn(B, STEP_Q, cfg.text_dim, generator=g).to(dev)
        qm_host = torch.rand(B, STEP_Q, generator=g) > 0.1
        qm_host[:, :NT] = True
        qm = qm_host.to(dev)
        xy = torch.rand(B, NT, 2, generator=g) * 0.6
        targets = [{"class_labels": torch.randint(0, NT, (NT,), generator=g), "boxes": torch.cat([xy[b], xy[b] + 0.05 + 0.3 * torch.rand(NT, 2, generator=g)], -1)}
                   for b in range(B)]
        crit = OpenVocabLoss()
        # both heads are built once; a form switches by handing the model the one it runs with (two attribute stores, nothing on the device)
        model.set_logit_head(head, trainable=True)
        trained_head = (model.logit_head, model._logit_head_flat)
        hopt = torch.optim.AdamW(model.logit_head_parameters(), lr=1e-4)
        model.set_logit_head(head)
        frozen_head = (model.logit_head, None)

        def step(which, head_opt):
            model.logit_head, model._logit_head_flat = which
            opt.zero_grad()
            if head_opt is not None:
                head_opt.zero_grad()
            pb, lg = model.forward_queries(img, qe, qm)
            o = crit(lg, pb, targets, query_mask=qm)
            (o["loss_ce"] + 5.0 * o["loss_bbox"] + 2.0 * o["loss_giou"]).backward()
            opt.step()
            if head_opt is not None:
                head_opt.step()

        forms = dict(frozen=lambda: step(frozen_head, None), trained=lambda: step(trained_head, hopt))
        model_res = dict(Q=STEP_Q, us=measure(forms, 3))
    print("RESULT " + json.dumps(dict(kernel=out, model=model_res)), flush=True)


def read_trace(folder, launches):
    """-> per Q: median us of ovb_rows_kernel without / with the rowgrad store, of ovb_head_part_kernel and of ovb_head_finish_kernel, over the timed
    dispatches (the last `launches` of each kind per Q)."""
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"]
                kind = next((k for k in ("ovb_rows_kernel", "ovb_head_part_kernel", "ovb_head_finish_kernel") if k in name), None)
                if kind:
                    rows.append((int(r["Start_Timestamp"]), kind, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    # per Q, in dispatch order: two warm-up calls of each entry (row pass | row pass, partial, final, twice), then `launches` calls of
    # owl_class_logits_bwd (a row pass each), then `launches` of owl_class_logits_bwd_head (row pass, partial, final each)
    per = 4 * (launches + 2)
    if len(rows) != per * len(QS):
        raise SystemExit(f"trace: {len(rows)} dispatches of this file's kernels, {per * len(QS)} expected")
    out = []
    for i in range(len(QS)):
        grp = rows[i * per:(i + 1) * per][8:]
        plain, head = grp[:launches], grp[launches:]
        want = ["ovb_rows_kernel"] * launches + ["ovb_rows_kernel", "ovb_head_part_kernel", "ovb_head_finish_kernel"] * launches
        if [k for _, k, _ in grp] != want:
            raise SystemExit("trace: the dispatches are not in the order the child launched them")
        med = lambda v: statistics.median(us for _, _, us in v)
        out.append(dict(rows=med(plain), rows_store=med(head[0::3]), ovb_head_part_kernel=med(head[1::3]), ovb_head_finish_kernel=med(head[2::3])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--limit", type=int, default=600, help="seconds for each child process")
    ap.add_argument("--no-model", action="store_true", help="the kernels only (skips building B/16 and the train-step rows)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run (the per-kernel rows are then `not measured`)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-trace", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.windows, args.launches, not args.no_model)
    if args.child_trace:
        return child_trace(args.launches)
    me = [sys.executable, os.path.abspath(__file__), "--launches", str(args.launches)]

    def run(cmd, want):
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"no result within {args.limit} s -- stopped: nothing more is started on the device")
        res = [ln for ln in r.stdout.splitlines() if ln.startswith(want)]
        if r.returncode != 0 or not res:
            sys.exit(f"exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-2000:]}\n-- stopped: nothing more is started on the device")
        return res[-1]

    line = run(me + ["--child", "--windows", str(args.windows)] + (["--no-model"] if args.no_model else []), "RESULT ")
    print(line, flush=True)
    data = json.loads(line[7:])
    trace = None
    if not args.no_trace:
        with tempfile.TemporaryDirectory() as tmp:
            run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--"] + me + ["--child-trace"], "TRACED")
            trace = read_trace(tmp, args.launches)
        print("TRACE " + json.dumps(trace), flush=True)
    f = lambda x: f"{x['median']:.1f} ({x['lo']:.1f} .. {x['hi']:.1f})"
    rows = B * P
    nbytes = rows * D * 2 + rows * 8
    lines = [f"`owl_class_logits_bwd_head` beside `owl_class_logits_bwd` at rows = {B} x {P}, Dt = {DT}, D = {D}, per-image banks and masks, dqueries NULL; us per "
             "call between HIP events, median (min .. max) of the windows", "",
             "| Q | `owl_class_logits_bwd` (head frozen) | `owl_class_logits_bwd_head` | difference | torch ops `rowgrad.T @ feats.float()` |", "|---|---|---|---|---|"]
    for o in data["kernel"]:
        u = o["us"]
        lines.append(f"| {o['Q']} | {f(u['frozen'])} | {f(u['trained'])} | {u['trained']['median'] - u['frozen']['median']:.1f} | {f(u['torch_product'])} |")
    lines += ["", f"Per kernel, from a `rocprofv3 --kernel-trace` run of its own (median us of {args.launches} dispatches); the reduction reads {nbytes / 1e6:.1f} MB "
              f"({rows} x {D} bf16 features + {rows} x 2 f32 row scalars) once; the LayerNorm kernels stream at {LN_STREAM_TBS} TB/s", "",
              "| Q | row pass, no `rowgrad` store | row pass, with the store | partial sums (`ovb_head_part_kernel`) | achieved TB/s | final sum (`ovb_head_finish_kernel`) |",
              "|---|---|---|---|---|---|"]
    for i, Q in enumerate(QS):
        if trace is None:
            lines.append(f"| {Q} | not measured | not measured | not measured | not measured | not measured |")
        else:
            t = trace[i]
            lines.append(f"| {Q} | {t['rows']:.1f} | {t['rows_store']:.1f} | {t['ovb_head_part_kernel']:.1f} | {nbytes / t['ovb_head_part_kernel'] / 1e6:.2f} | "
                         f"{t['ovb_head_finish_kernel']:.1f} |")
    if data["model"]:
        m = data["model"]
        lines += ["", f"Train step on owlvit-base-patch16, batch {B}, bf16 images, the default trainable set, `forward_queries` + `OpenVocabLoss`, {m['Q']} queries per "
                  "image, FusedAdamW in-line (trained: plus a `torch.optim.AdamW` over `logit_head_parameters()`); us per step", "",
                  "| head frozen (today's launches) | head trained |", "|---|---|", f"| {f(m['us']['frozen'])} | {f(m['us']['trained'])} |"]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
