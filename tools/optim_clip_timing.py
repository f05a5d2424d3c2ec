"""HIP-event medians of the optimizer entries at the B/16 bucket size (profiles/optim_clip.md): owl_adamw_step, owl_grad_sumsq and
owl_adamw_step_grouped (two groups: no decay for LayerNorm affines, biases and the query bank) with and without clipping, on raw buffers.
  python tools/optim_clip_timing.py [--parent-lib PATH/libowlhip.so] [--out FILE.json]
--parent-lib: a library built from another commit; its owl_adamw_step is timed in the same process, alternated with this tree's."""
import argparse, ctypes, json, os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: F401  (the importable alias of the package directory)
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
from owl_vit_object_detection_amd import weights, models
from owl_vit_object_detection_amd.config import get_config

cfg = get_config("owlvit-base-patch16")
shapes = weights.param_shapes(cfg)
offs, off = {}, 0
for nme in models._flat_order(cfg):
    offs[nme] = off; off += (int(np.prod(shapes[nme])) + 7) // 8 * 8
n = off
names = list(offs)
nd = lambda x: x.endswith(".bias") or "layer_norm" in x or "layernorm" in x or x == "queries"
segs = []
for k, nme in enumerate(names):
    end = offs[names[k + 1]] if k + 1 < len(names) else n
    gi = 1 if nd(nme) else 0
    if segs and segs[-1][1] == gi: segs[-1] = (end, gi)
    else: segs.append((end, gi))
print("n", n, "segments", len(segs), flush=True)

V, I64, F, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
def load(path):
    lib = ctypes.CDLL(path)
    lib.owl_adamw_step.argtypes = [V, V, V, V, V, V, I64, F, F, F, F, F, I64, F]; lib.owl_adamw_step.restype = I
    return lib
new = load(os.path.join(ROOT, "owl-vit-object-detection_amd", "libowlhip.so"))
old = load(args.parent_lib) if args.parent_lib else None
new.owl_grad_sumsq.argtypes = [V, V, I64, V]; new.owl_grad_sumsq.restype = I
new.owl_grad_norm_workspace_bytes.argtypes = [I64, V]; new.owl_grad_norm_workspace_bytes.restype = I
new.owl_adamw_step_grouped.argtypes = [V, V, V, V, V, V, I64, F, F, F, F, F, I64, F, V, V, V, I, F, V, V]; new.owl_adamw_step_grouped.restype = I

dev = "cuda"
gen = torch.Generator(device=dev).manual_seed(0)
p = torch.randn(n, device=dev, generator=gen) * 0.02
g = torch.randn(n, device=dev, generator=gen) * 1e-3
m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev); pb = torch.zeros(n, device=dev, dtype=torch.bfloat16)
nb = torch.zeros(1, dtype=torch.int64); assert new.owl_grad_norm_workspace_bytes(n, nb.data_ptr()) == 0
ws = torch.zeros(int(nb.item()) // 8, dtype=torch.float64, device=dev); norm = torch.zeros((), device=dev)
end = torch.tensor([e for e, _ in segs], dtype=torch.int64)
lr = torch.tensor([3e-6 if gi == 0 else 1.5e-6 for _, gi in segs], dtype=torch.float32)
wd = torch.tensor([0.1 if gi == 0 else 0.0 for _, gi in segs], dtype=torch.float32)
st = torch.cuda.current_stream().cuda_stream
P = lambda t: t.data_ptr()
step = [0]
def adamw(lib):
    step[0] += 1
    return lib.owl_adamw_step(st, P(p), P(g), P(m), P(v), P(pb), n, 3e-6, 0.9, 0.999, 1e-8, 0.1, step[0], 1.0)
def grouped(mx):
    step[0] += 1
    return new.owl_adamw_step_grouped(st, P(p), P(g), P(m), P(v), P(pb), n, 3e-6, 0.9, 0.999, 1e-8, 0.1, step[0], 1.0, P(end), P(lr), P(wd), len(segs), mx,
                                      P(ws) if mx > 0 else None, P(norm) if mx > 0 else None)
def both():
    rc = new.owl_grad_sumsq(st, P(g), n, P(ws))
    return rc or grouped(1e-3)
ops_ = {"owl_adamw_step (parent)": lambda: adamw(old), "owl_adamw_step (this commit)": lambda: adamw(new),
        "owl_grad_sumsq": lambda: new.owl_grad_sumsq(st, P(g), n, P(ws)), "owl_adamw_step_grouped, 2 groups, no clip": lambda: grouped(0.0),
        "owl_adamw_step_grouped, 2 groups, clip (partials ready)": lambda: grouped(1e-3),
        "owl_grad_sumsq + owl_adamw_step_grouped, clip (one event pair)": both}
if old is None:
    del ops_["owl_adamw_step (parent)"]
times = {k: [] for k in ops_}
for rnd in range(6):                      # round 0 = warm-up
    for k, f in ops_.items():
        evs = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); rc = f(); b.record()
            assert rc == 0, (k, rc)
            evs.append((a, b))
        torch.cuda.synchronize()
        if rnd:
            times[k] += [a.elapsed_time(b) * 1e3 for a, b in evs]
out = {k: dict(median_us=round(statistics.median(t), 2), min_us=round(min(t), 2), p90_us=round(sorted(t)[int(0.9 * len(t))], 2), launches=len(t)) for k, t in times.items()}
out["n"] = n; out["segments"] = len(segs); out["last_grad_norm"] = float(norm); out["norm_f64"] = float(torch.sqrt((g.double() ** 2).sum()))
print(json.dumps(out, indent=1))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
