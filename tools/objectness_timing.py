"""What OWLv2's objectness head costs on the card, beside the box head's same sections (recorded, not asserted; profiles/objectness.md).
  python tools/objectness_timing.py [--out profiles/objectness.md] [--rounds 7] [--launches 400] [--limit 400] [--parent DIR]
Geometry: owlv2-base-patch16 at batch 32 -- 115 200 rows (32 x 3600 patches), D = 768; random bf16 activations resident in HBM (the kernels' time does not
depend on the values).  Every launch of the forward (two erf-GELU GEMMs, the row-dot tail) and of the backward chain (tail backward, dense1's weight
gradient, the dX GEMM through GELU', dense0's weight and bias gradient) is timed on its own between two HIP events around `--launches` back-to-back calls (five times as many for the four
tail kernels, so that every timed window is tens of milliseconds), 10 warm-up calls, `--rounds` rounds with the objectness and box launches alternated,
median (min .. max).  The forward tails read one of FOUR input buffers in turn (4 x 177 MB, beyond the 256 MiB Infinity Cache), so their rate is an HBM
streaming rate, not a warm-cache one; a backward tail moves 550 MB per launch on its own.  The GEMM and weight-gradient launches are the
SAME launches for both heads (same shapes, same epilogues), so they are timed once; the tails differ.  Bytes are the compulsory traffic from the shapes.
`--parent DIR` (a checkout of the parent commit with its library built) adds the default benchmark line, `bench.py --gpus 1 --steps 20 --warmup 5 --windows 5`,
alternated between that tree and this one: the head launches nothing there, so the two must agree within the window spread.
One fresh child process per measurement under its own time limit; a child that fails ends the run: nothing more is started on the device."""
import argparse, json, os, statistics, subprocess, sys
from types import SimpleNamespace
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)

B, P, D = 32, 3600, 768
ROWS = B * P
LN_STREAM_TBS = 6.2          # what the LayerNorm kernels stream at (profiles/r06_README.md): the yardstick for a kernel bound by one read


def child(rounds, launches):
    import torch
    from owl_vit_object_detection_amd import autograd, ops
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(0)
    bf = lambda *s: ops.zeros_rows(s[0], s[1], torch.bfloat16, dev).copy_(torch.randn(ops.pad_rows(s[0]), s[1], generator=g).to(dev)) if len(s) == 2 else None
    feats, h0, u0, h1, u1, du1, du0 = (bf(ROWS, D) for _ in range(7))
    W = (D ** -0.5 * torch.randn(D, D, generator=g)).to(dev).to(torch.bfloat16)
    WT = torch.empty_like(W)
    bias = (0.02 * torch.randn(D, generator=g)).to(dev)
    w2o, b2o = (D ** -0.5 * torch.randn(D, generator=g)).to(dev), torch.tensor([-1.0], device=dev)
    w2b, b2b = (D ** -0.5 * torch.randn(4, D, generator=g)).to(dev), torch.zeros(4, device=dev)
    box_bias, boxes, sig = torch.zeros(P, 4, device=dev), torch.empty(ROWS, 4, device=dev), torch.empty(ROWS, 4, device=dev)
    h1s = [h1] + [h1.clone() for _ in range(3)]          # the forward tails' input in turn: no launch finds its rows in the Infinity Cache
    turn = [0]

    def next_h1():
        turn[0] = (turn[0] + 1) % len(h1s)
        return h1s[turn[0]]
    logits, dlog, dbox = torch.empty(ROWS, device=dev), torch.randn(ROWS, generator=g).to(dev), torch.randn(ROWS, 4, generator=g).to(dev)
    stub = SimpleNamespace(cfg=SimpleNamespace(hidden=D, patches=P), device_=torch.device(dev), _ws={})
    bw = autograd._objectness_bws(stub, B)
    gW, gb = torch.zeros(D, D, device=dev), torch.zeros(D, device=dev)
    g2o, colsum = torch.zeros(D + 4, device=dev), torch.zeros(D, device=dev)
    g2b = torch.zeros(4 * D + 4, device=dev)
    from owl_vit_object_detection_amd import _lib
    part_box = torch.zeros(_lib.load().owl_box_final_bwd_blocks(ROWS), 5 * D + 4, device=dev)
    forms = {
        "gemm_gelu": lambda: ops.gemm(ops.EPI_GELU_BF16, feats, W, h0, bias=bias, aux=u0, M=ROWS, N=D, K=D),
        "obj_final": lambda: ops.objectness_final(next_h1(), w2o, b2o, logits, ROWS, D),
        "box_final": lambda: ops.box_final(next_h1(), w2b, b2b, box_bias, boxes, sig, ROWS, P, D),
        "obj_final_bwd": lambda: ops.objectness_final_bwd(dlog, h1, u1, w2o, du1, bw["part"], g2o, ROWS, D, du1_colsum=colsum),
        "box_final_bwd": lambda: ops.box_final_bwd(dbox, sig, h1, u1, w2b, du1, part_box, g2b, ROWS, D, du1_colsum=colsum),
        "dw": lambda: autograd.weight_grad(du1, h0, gW, D, D, ROWS, bw["dw"], accumulate=0),
        "dx_dgelu": lambda: (ops.transpose_bf16(W, WT, D, D), ops.gemm(ops.EPI_DGELU_BF16, du1, WT, du0, aux=u0, M=ROWS, N=D, K=D)),
        "dw_bias": lambda: autograd.weight_grad(du0, feats, gW, D, D, ROWS, bw["dw"], gb, accumulate=0),
    }

    def between_events(fn, n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    ops.box_final(h1, w2b, b2b, box_bias, boxes, sig, ROWS, P, D)          # a finite sig for the box tail's backward
    for fn in forms.values():
        between_events(fn, 10)
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(between_events(fn, launches * (5 if "final" in k else 1)))
    nblk_o, nblk_b = bw["part"].shape[0], part_box.shape[0]
    by = {"obj_final": ROWS * D * 2 + ROWS * 4, "box_final": ROWS * D * 2 + ROWS * 32,
          "obj_final_bwd": 3 * ROWS * D * 2 + ROWS * 4 + 2 * nblk_o * (2 * D + 4) * 4, "box_final_bwd": 3 * ROWS * D * 2 + ROWS * 32 + 2 * nblk_b * (5 * D + 4) * 4}
    res = dict(rounds=rounds, launches=launches, ms={k: dict(median=statistics.median(v), lo=min(v), hi=max(v)) for k, v in ms.items()}, bytes=by)
    print("RESULT " + json.dumps(res), flush=True)


def table(o):
    m = o["ms"]
    f = lambda k: f"{m[k]['median']:.4f} ({m[k]['lo']:.4f}–{m[k]['hi']:.4f})"
    med = lambda k: m[k]["median"]
    bw = lambda k: o["bytes"][k] / (med(k) * 1e-3) / 1e12
    fo, fb = 2 * med("gemm_gelu") + med("obj_final"), 2 * med("gemm_gelu") + med("box_final")
    chain = med("dw") + med("dx_dgelu") + med("dw_bias")
    lines = ["# OWLv2's objectness head on one MI355X", "", "Written by `tools/objectness_timing.py`; recorded, not asserted anywhere.", "",
             f"owlv2-base-patch16 at batch {B}: {ROWS} rows, D = {D}.  ms per launch, median (min–max).", "",
             "| section | objectness head | box head |", "|---|---|---|",
             f"| forward: dense0 / dense1 GEMM + erf-GELU, pre-activation saved (each; the same launch for both heads) | {f('gemm_gelu')} | same launch |",
             f"| forward: tail (`owl_objectness_final_fwd` / `owl_box_final_fwd`) | {f('obj_final')} | {f('box_final')} |",
             f"| forward, three launches | {fo:.4f} | {fb:.4f} |",
             f"| backward: tail (`owl_objectness_final_bwd` / `owl_box_final_bwd`, reduces included) | {f('obj_final_bwd')} | {f('box_final_bwd')} |",
             f"| backward: dense1 weight gradient (`weight_grad`, D x D) | {f('dw')} | same launch |",
             f"| backward: transpose of W1 + dX GEMM through GELU' | {f('dx_dgelu')} | same launch |",
             f"| backward: dense0 weight + bias gradient | {f('dw_bias')} | same launch |",
             f"| backward chain (no dX GEMM into feats for objectness: HF detaches) | {med('obj_final_bwd') + chain:.4f} | {med('box_final_bwd') + chain:.4f} + its dX GEMM into feats |",
             "", "| tail kernel | compulsory bytes | achieved | share of the 6.2 TB/s the LayerNorm kernels stream at |", "|---|---|---|---|"]
    for k, name in (("obj_final", "objectness forward"), ("box_final", "box forward"), ("obj_final_bwd", "objectness backward"), ("box_final_bwd", "box backward")):
        lines.append(f"| {name} | {o['bytes'][k] / 1e6:.1f} MB | {bw(k):.2f} TB/s | {100 * bw(k) / LN_STREAM_TBS:.0f} % |")
    lines += ["", f"Median (min–max) of {o['rounds']} rounds of {o['launches']} back-to-back launches (tails: {5 * o['launches']}) between two HIP events, 10 warm-up launches each, "
              "all launches alternated in one process.  Bytes: the forward tails read rows x D bf16 once and write the row results; the backward tails read h1 and u1, write du1 and "
              "write and re-read their partials.  The backward tails' time includes their slab reduces.  The forward tails read four 177 MB inputs in turn (708 MB, beyond the 256 MiB "
              "Infinity Cache): their figures are HBM streaming rates; a backward tail moves 550 MB per launch.", ""]
    return "\n".join(lines)


def bench_line(tree, limit):
    tree = os.path.abspath(tree)
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--windows", "5", "--no-cpu-baseline", "--no-compare"]
    try:
        out = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench.py in {tree}: no result within {limit} s -- stopped: nothing more is started on the device")
    if out.returncode != 0:
        sys.exit(f"bench.py in {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}\n-- stopped: nothing more is started on the device")
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return dict(value=line["value"], windows=line["config"]["window_values"], spread=line["config"]["window_spread_pct"])


def bench_ab(parent, rounds, limit):
    runs = []
    for _ in range(rounds):
        for name, tree in (("parent", parent), ("this tree", ROOT)):
            runs.append((name, bench_line(tree, limit)))
            print(name, runs[-1][1], flush=True)
    md = ["## The default benchmark (768 x 768, B/16, batch 32): this tree against the parent commit", "",
          "`bench.py --gpus 1 --steps 20 --warmup 5 --windows 5`, alternating, same session, same card.  The objectness head launches nothing here.", "",
          "| run | tree | images/s (median window) | windows | window spread % |", "|---|---|---|---|---|"]
    for i, (name, b) in enumerate(runs):
        md.append(f"| {i} | {name} | {b['value']:.2f} | {b['windows']} | {b['spread']:.2f} |")
    p = statistics.median(b["value"] for n, b in runs if n == "parent")
    t = statistics.median(b["value"] for n, b in runs if n == "this tree")
    md += ["", f"Median of the runs: parent {p:.2f}, this tree {t:.2f} images/s: {100.0 * (t - p) / p:+.2f} % (largest window spread of a run: "
               f"{max(b['spread'] for _, b in runs):.2f} %).", ""]
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: adds the default benchmark, alternated")
    ap.add_argument("--ab-rounds", type=int, default=3, help="alternations parent / this tree")
    ap.add_argument("--limit", type=int, default=400, help="seconds for the child process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.rounds, args.launches)
        return
    argv = ["--child", "--rounds", str(args.rounds), "--launches", str(args.launches)]
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"no result within {args.limit} s -- stopped: nothing more is started on the device")
    res = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        sys.exit(f"exit {r.returncode}\n{r.stderr[-3000:]}\n-- stopped: nothing more is started on the device")
    print(res[-1], flush=True)
    text = table(json.loads(res[-1][7:]))
    if args.parent:
        text += "\n" + bench_ab(args.parent, args.ab_rounds, args.limit)
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
