"""-m gpu: OWLv2's input stage on a real MI355X -- DeviceImageProcessor(resize="owlv2") = owl_pad_resize_coeffs + owl_preprocess_u8_pad_resize
(csrc/pad_resize.hip) -- against the float64 restatement of tests/owlv2_input_reference.py, every element inside the bound derived there from the kernels'
evaluation order, on the sources of fixture F19 (tests/golden/make_golden_owlv2.py).  Imports neither scipy nor transformers.

Shapes: the smallest that reach every path -- pad on either side, no pad, pad only (S = N), upsampling with the mirror at the far edge, one padded
column, a one-row image, an odd N-multiple width, and S = 16 N (62 taps, the limit).  Each test prints its worst err / tol;
profiles/owlv2_input_reference.md records them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import _lib, ops, weights  # noqa: E402
from owl_vit_object_detection_amd.config import get_config, get_text_config  # noqa: E402
from owl_vit_object_detection_amd.models import OwlViT  # noqa: E402
from owl_vit_object_detection_amd.postprocess import unpad_boxes  # noqa: E402
from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor, DevicePrefetcher, TrainAugment  # noqa: E402
from tests import owlv2_input_reference as R  # noqa: E402
from tests.golden.make_golden_open_vocab import D_BOXES, model_tolerance  # noqa: E402
from tests.golden.make_golden_owlv2 import v2_state_dict  # noqa: E402

DEV = "cuda"
N_BATCH = 24          # the one size every case fits under S <= 16 N (384 = 16 x 24)


@pytest.fixture(scope="module")
def f19(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "f19_owlv2_input.npz")))


@pytest.fixture(scope="module")
def sources(f19):
    return [torch.from_numpy(f19["src/" + R.case_key(*c)]).to(DEV) for c in R.CASES]


def _proc(N, dtype=torch.float32, pad=0.0):
    return DeviceImageProcessor(N, device=DEV, dtype=dtype, resize="owlv2", pad_value=pad)


def _launch(proc, imgs, out, tmp):
    """The C entry on the caller's own `out` and `tmp` (the processor's descriptors and tables)."""
    rows, tmp_bytes, max_h = proc._pad_resize_plan(imgs)
    assert tmp.numel() * 4 >= tmp_bytes
    desc = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(DEV)
    N = proc.hw[0]
    _lib.call("owl_preprocess_u8_pad_resize", ops.stream(), desc, len(imgs), max_h, tmp, proc._norm, proc.pad_value, out, 1 if proc.dtype == torch.bfloat16 else 0, N, N)
    torch.cuda.synchronize()
    return tmp_bytes


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_every_element_inside_the_bound(f19, case):
    H, W, N = case
    img = f19["src/" + R.case_key(H, W, N)]
    d = torch.from_numpy(img).to(DEV)
    for pad in (0.0, 0.5):
        o32 = _proc(N, torch.float32, pad)(d)["pixel_values"]
        obf = _proc(N, torch.bfloat16, pad)(d)["pixel_values"]
        torch.cuda.synchronize()
        assert o32.shape == (1, 3, N, N) and o32.dtype == torch.float32 and obf.dtype == torch.bfloat16
        r32 = R.check(f"({H},{W})->{N} pad {pad} f32", o32[0].cpu().numpy(), img, N, pad)
        rbf = R.check(f"({H},{W})->{N} pad {pad} bf16", obf[0].float().cpu().numpy(), img, N, pad, bf16=True)
        assert torch.equal(obf, o32.to(torch.bfloat16))          # the bf16 store is the f32 result rounded to nearest even
        print(f"({H},{W})->{N} pad {pad}: worst err / tol f32 {r32[0]:.3f} (max err {r32[1]:.2e}, max tol {r32[2]:.2e}); bf16 {rbf[0]:.3f} (max tol {rbf[2]:.2e})")
    if pad == 0.0 or H == W:
        return
    assert not torch.equal(o32, _proc(N)(d)["pixel_values"])          # the pad value reaches the output of a padded image


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ragged_batch_is_each_image_alone(sources, dtype):
    """Two runs give the same bits; an image alone gives the bits it has anywhere in one ragged batch of all eleven (either order)."""
    proc = _proc(N_BATCH, dtype, 0.5)
    a = proc(sources)["pixel_values"].clone()
    b = proc(sources)["pixel_values"].clone()
    rev = proc(sources[::-1])["pixel_values"].clone()
    torch.cuda.synchronize()
    assert a.shape == (len(sources), 3, N_BATCH, N_BATCH) and torch.equal(a, b) and torch.equal(rev.flip(0), a)
    fresh = _proc(N_BATCH, dtype, 0.5)          # a processor that has seen nothing else
    for k, s in enumerate(sources):
        assert torch.equal(fresh(s)["pixel_values"][0], a[k]), R.CASES[k]
    for k, c in enumerate(R.CASES):             # and the batch is inside the bound too, at the batch's size
        R.check(f"batch image {c}", a[k].float().cpu().numpy(), sources[k].cpu().numpy(), N_BATCH, 0.5, bf16=dtype == torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_writes_all_of_out_reads_only_what_it_wrote(sources, dtype):
    """`out` and `tmp` pre-filled with NaN: the result is the bits of a run on zeroed buffers (so every element of out is written and nothing of tmp is
    read that the launch did not write), and the guard elements behind out are untouched."""
    proc = _proc(N_BATCH, dtype, 0.5)
    n, GUARD = len(sources), 256
    numel = n * 3 * N_BATCH * N_BATCH
    tmp_bytes = proc._pad_resize_plan(sources)[1]
    outs = []
    for fill in (float("nan"), 0.0):
        buf = torch.full((numel + GUARD,), fill, dtype=dtype, device=DEV)
        buf[numel:] = 7.0
        tmp = torch.full((tmp_bytes // 4 + GUARD,), fill, dtype=torch.float32, device=DEV)
        _launch(proc, sources, buf, tmp)
        assert not torch.isnan(buf[:numel]).any()
        assert torch.equal(buf[numel:], torch.full((GUARD,), 7.0, dtype=dtype, device=DEV))
        assert torch.equal(torch.isnan(tmp[tmp_bytes // 4:]), torch.full((GUARD,), fill != 0.0, device=DEV))          # nothing written behind tmp either
        outs.append(buf[:numel].clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0].view(n, 3, N_BATCH, N_BATCH), proc(sources)["pixel_values"])


def test_pillow_mode_is_untouched(sources):
    """resize="pillow" (the default) still gives the bits of owl_preprocess_u8_batch."""
    N = N_BATCH
    default, named = DeviceImageProcessor(N, device=DEV), DeviceImageProcessor(N, device=DEV, resize="pillow")
    assert default.resize == "pillow" and default._norm is None
    a, b = default(sources)["pixel_values"], named(sources)["pixel_values"]
    rows, off = [], 0
    for im in sources:
        H, W = int(im.shape[0]), int(im.shape[1])
        bx, kx, ksx = default._axis_tables(W, N)
        by, ky, ksy = default._axis_tables(H, N)
        rows.append((im.data_ptr(), H, W, bx.data_ptr(), kx.data_ptr(), ksx, by.data_ptr(), ky.data_ptr(), ksy, off))
        off += (H * N * 3 + 255) // 256 * 256
    out = torch.empty(len(sources), 3, N, N, dtype=torch.float32, device=DEV)
    tmp = torch.empty(off, dtype=torch.uint8, device=DEV)
    desc = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(DEV)
    _lib.call("owl_preprocess_u8_batch", ops.stream(), desc, len(sources), max(int(s.shape[0]) for s in sources), tmp, default.lut, out, 0, N, N)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), out.cpu().numpy()) and np.array_equal(b.cpu().numpy(), out.cpu().numpy())
    assert not torch.equal(_proc(N)(sources)["pixel_values"], a)


def test_limits_raise_and_launch_nothing(sources):
    proc = _proc(16)
    big = torch.zeros(257, 8, 3, dtype=torch.uint8, device=DEV)          # S = 257 > 16 x 16
    with pytest.raises(ValueError, match="16 x the model size"):
        proc([sources[2], big])                                         # a good image first: the check runs before anything is built or launched
    assert proc._tmp_f32 is None and not proc._pad_tables and not hasattr(proc, "_keep")
    edge = torch.zeros(256, 8, 3, dtype=torch.uint8, device=DEV)         # S = 16 N: allowed
    assert proc(edge)["pixel_values"].shape == (1, 3, 16, 16)
    with pytest.raises(ValueError, match="square"):
        DeviceImageProcessor((16, 24), device=DEV, resize="owlv2")
    with pytest.raises(ValueError, match="resize"):
        DeviceImageProcessor(16, device=DEV, resize="bilinear")
    with pytest.raises(ValueError, match="pad_value"):
        DeviceImageProcessor(16, device=DEV, resize="owlv2", pad_value=128)
    for call in (lambda: proc.tiles(sources[:1], [], 1), lambda: proc.slices(sources[:1]), lambda: proc.run_tiles(None, 1, 1, 1, 1)):
        with pytest.raises(ValueError, match="owlv2"):
            call()
    with pytest.raises(ValueError, match="owlv2"):
        DevicePrefetcher([], DEV, size=16, dtype=torch.float32, processor=proc, augment=TrainAugment(16))


def test_normalize_sized_is_the_stage_at_the_model_size(f19):
    """At S = N with no pad every tap is 1.0, so HF's stage is the table step: normalize_sized stays allowed in this mode and gives HF's own bits (its
    float32 rescale and normalise), while the kernel's one affine step sits inside its bound."""
    img = f19["src/16x16_16"]
    proc = _proc(16)
    d = torch.from_numpy(img).to(DEV)
    assert np.array_equal(proc.normalize_sized(d[None], chw=False)[0].cpu().numpy(), f19["pv/16x16_16"])
    R.check("kernel at S = N", proc(d)["pixel_values"][0].cpu().numpy(), img, 16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("threaded", [False, True])
def test_through_the_prefetcher(f19, sources, dtype, threaded):
    host = [torch.from_numpy(f19["src/" + R.case_key(*c)]) for c in R.CASES]
    proc = _proc(N_BATCH, dtype)
    direct = proc(sources)["pixel_values"].clone()
    loader = [(host, torch.arange(3)), (host[::-1], torch.arange(4))]
    got = [(img.clone(), t) for img, t in DevicePrefetcher(loader, DEV, size=N_BATCH, dtype=dtype, processor=proc, threaded=threaded)]
    torch.cuda.synchronize()
    assert len(got) == 2 and got[0][0].dtype == dtype
    assert torch.equal(got[0][0], direct) and torch.equal(got[1][0], direct.flip(0))
    assert torch.equal(got[1][1].cpu(), torch.arange(4))


def test_model_on_v2_names_against_hf(f19):
    """F19's model case: HF's Owlv2ForObjectDetection at `tiny` on HF's processor output of a 70 x 100 image; here the u8 image through the device stage,
    the same weights through the `owlv2.` names, set_logit_head, detect.  Logits inside make_golden_open_vocab.model_tolerance, boxes under D_BOXES, and
    unpad_boxes of the result on HF's post-processed pixel boxes within that bar times max(h, w)."""
    g = f19
    cfg, tc = get_config("tiny"), get_text_config("tiny")
    sd = v2_state_dict(cfg, tc)
    sd.update({"class_head." + k: g["head/" + k] for k in weights.LOGIT_HEAD_KEYS})
    state = weights.from_hf_state_dict(sd, queries=weights.make_weights(cfg)["queries"])
    assert any(k.startswith("backbone.") for k in state) and not any("objectness" in k for k in state)
    model = OwlViT(cfg, state, DEV)
    head = weights.hf_logit_head(sd)
    model.set_logit_head(head)
    H, W = (int(v) for v in g["m_size"])
    pv = _proc(cfg.image_size)(torch.from_numpy(g["m_src"]).to(DEV))["pixel_values"]
    r = R.check("model case input", pv[0].cpu().numpy(), g["m_src"], cfg.image_size)
    d_in = float(np.abs(pv[0].cpu().numpy() - g["m_pixel_values"]).max())
    boxes, logits = model.detect(pv, torch.from_numpy(g["m_text_embeds"]).to(DEV))
    torch.cuda.synchronize()
    ref = g["m_logits"].astype(np.float64)
    f = torch.from_numpy(g["m_image_embeds"]).double()
    x = f @ torch.from_numpy(head["logit_scale.weight"]).double() + float(head["logit_scale.bias"])
    scale = (torch.where(x > 0, x, torch.expm1(x)) + 1.0)[..., None].numpy()
    tol = model_tolerance(scale, ref / scale, head["logit_shift.weight"], head["logit_scale.weight"])
    err = np.abs(logits.cpu().double().numpy() - ref)
    cx, cy, w, h = (g["m_pred_boxes"][..., k] for k in range(4))
    corners = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    eb = float(np.abs(boxes.cpu().numpy() - corners).max())
    px = unpad_boxes(boxes, [(H, W)], to="pixels")
    ep = float(np.abs(px[0].cpu().numpy() - g["m_pp_boxes"]).max())
    print(f"model case ({H},{W})->{cfg.image_size}: input err / tol {r[0]:.3f}, max |input - HF's| {d_in:.2e}; max |d logit| {err.max():.3e}, worst err / tol "
          f"{(err / tol).max():.3f}; max |d boxes| {eb:.3e} (bar {D_BOXES}); max |d pixel boxes| {ep:.3e} (bar {D_BOXES * max(H, W):.2f})")
    assert logits.shape == ref.shape and (err / tol).max() <= 1.0
    assert eb < D_BOXES
    assert ep < D_BOXES * max(H, W)
    nb = unpad_boxes(boxes, [(H, W)], to="normalized")          # x in units of the width, y of the height
    assert torch.allclose(nb[..., 0::2] * W, px[..., 0::2], rtol=1e-6, atol=1e-4) and torch.allclose(nb[..., 1::2] * H, px[..., 1::2], rtol=1e-6, atol=1e-4)
