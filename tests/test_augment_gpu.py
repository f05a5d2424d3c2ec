"""Train-time augmentation on the device: `owl_preprocess_u8_tiles` against the numpy restatement of Pillow's boxed resize / flip / paste
(tests/augment_reference.py, pinned to PIL by tests/test_augment.py), bit for bit, f32 and bf16, at mosaic grids 1, 2 and 3 -- and the same through
`DevicePrefetcher(augment=TrainAugment(...))`.  Sources of 37x53, 64x48 and 20x31 into 24 x 24 canvases: the smallest shapes that reach fractional boxes,
boxes flush with each border, a row range that excludes the first and last source rows, ksize 13 down-scales and up-scales."""
import numpy as np
import pytest
import torch

from tests import augment_reference as R

pytestmark = pytest.mark.gpu

SRC = R.sources()
_REF = {}


def _ref(name):
    """f32 [n,3,S,S] reference pixel_values of a case, computed once."""
    if name not in _REF:
        tiles, n_out = R.cases()[name]
        _REF[name] = torch.from_numpy(R.pixel_values(R.render(SRC, tiles, n_out, R.SIZE)))
    return _REF[name]


def _ptiles(tiles):
    from owl_vit_object_detection_amd.preprocess import Tile
    return [Tile(*t) for t in tiles]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["single", "mixed"])
def test_tiles_equal_the_restatement(name, dtype):
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    tiles, n_out = R.cases()[name]
    ip = DeviceImageProcessor(size=R.SIZE, dtype=dtype)
    got = ip.tiles(SRC, _ptiles(tiles), n_out)
    assert got.dtype == dtype and tuple(got.shape) == (n_out, 3, R.SIZE, R.SIZE)
    assert torch.equal(got.cpu(), _ref(name).to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_identity_tiles_are_the_plain_batch_path(dtype):
    """Full box, g = 1, no flip: bitwise owl_preprocess_u8_batch."""
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor, Tile
    ip = DeviceImageProcessor(size=R.SIZE, dtype=dtype)
    plain = ip(images=SRC)["pixel_values"].clone()
    tiles = [Tile(k, (0.0, 0.0, float(W), float(H)), False, k, 0, 0, R.SIZE, R.SIZE) for k, (H, W) in enumerate(R.SHAPES)]
    assert torch.equal(ip.tiles(SRC, tiles, len(SRC)), plain)


def test_tile_order_does_not_change_the_bits():
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    tiles, n_out = R.cases()["mixed"]
    ip = DeviceImageProcessor(size=R.SIZE, dtype=torch.float32)
    perm = np.random.default_rng(0).permutation(len(tiles))
    assert not np.array_equal(perm, np.arange(len(tiles)))
    got = ip.tiles(SRC, [_ptiles(tiles)[i] for i in perm], n_out)
    assert torch.equal(got.cpu(), _ref("mixed"))
    got = ip.tiles(SRC, _ptiles(tiles)[::-1], n_out)
    assert torch.equal(got.cpu(), _ref("mixed"))


def test_tiles_that_do_not_cover_the_canvas_raise():
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    tiles, n_out = R.cases()["mixed"]
    ip = DeviceImageProcessor(size=R.SIZE, dtype=torch.float32)
    with pytest.raises(ValueError, match="cover"):
        ip.tiles(SRC, _ptiles(tiles)[:-1], n_out)
    with pytest.raises(ValueError, match="overlap"):
        ip.tiles(SRC, _ptiles(tiles)[:-1] + [_ptiles(tiles)[-2]], n_out)
    with pytest.raises(ValueError, match="box"):
        ip.tiles(SRC, [_ptiles(tiles)[0]._replace(box=(0.0, 0.0, 32.0, 17.0))], 1)


# ---- through the prefetcher ------------------------------------------------------------------------------------------------------------------------
def _targets():
    boxes = [torch.tensor([[W / 4, H / 4, W / 2, H / 2]], dtype=torch.float32) for H, W in R.SHAPES]      # COCO xywh pixels: the central quarter
    labels = [torch.tensor([k]) for k in range(len(R.SHAPES))]
    return labels, boxes


def _loader(n_batches):
    labels, boxes = _targets()
    for i in range(n_batches):
        yield [torch.from_numpy(im) for im in SRC], labels, boxes, {"batch": i}


def _augment(**kw):
    from owl_vit_object_detection_amd.preprocess import TrainAugment
    return TrainAugment(R.SIZE, mosaic=(1, 2, 3), seed=21, **kw)


@pytest.mark.parametrize("threaded", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prefetcher_batch_is_the_sampler_plus_the_restatement(dtype, threaded):
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher
    aug = _augment()
    pf = DevicePrefetcher(_loader(3), "cuda", size=R.SIZE, dtype=dtype, augment=aug, threaded=threaded)
    pf.set_epoch(4)
    by_hand = _augment()
    labels, boxes = _targets()
    grids, n = set(), 0
    for i, (img, lab, box, meta) in enumerate(pf):
        tiles, ob, ol = by_hand.sample(R.SHAPES, [b.numpy() for b in boxes], [l.numpy() for l in labels], 4, i)
        grids |= {R.SIZE // t.cw for t in tiles}
        exp = torch.from_numpy(R.pixel_values(R.render(SRC, tiles, len(SRC), R.SIZE))).to(dtype)
        assert img.is_cuda and img.dtype == dtype and torch.equal(img.cpu(), exp)
        assert meta == {"batch": i}
        for j in range(len(SRC)):
            assert lab[j].is_cuda and box[j].is_cuda and box[j].dtype == torch.float32 and len(box[j]) >= 1
            assert np.array_equal(box[j].cpu().numpy(), ob[j]) and np.array_equal(lab[j].cpu().numpy(), ol[j])
        n += 1
    assert n == 3 and len(grids) > 1 and aug.fallbacks == 0


def test_prefetcher_same_seed_and_epoch_same_bits():
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher

    def run(epoch, threaded):
        pf = DevicePrefetcher(_loader(2), "cuda", size=R.SIZE, dtype=torch.float32, augment=_augment(), threaded=threaded)
        pf.set_epoch(epoch)
        return [(img.cpu(), [b.cpu() for b in box], [l.cpu() for l in lab]) for img, lab, box, _ in pf]

    a, b, c = run(1, True), run(1, False), run(2, True)
    for (ia, ba, la), (ib, bb, lb) in zip(a, b):
        assert torch.equal(ia, ib) and all(torch.equal(x, y) for x, y in zip(ba, bb)) and all(torch.equal(x, y) for x, y in zip(la, lb))
    assert not all(torch.equal(x[0], y[0]) for x, y in zip(a, c))                   # another epoch draws other crops
    assert not torch.equal(a[0][0], a[1][0])                                         # ... and so does the next batch of the same epoch


def test_prefetcher_without_augment_is_the_plain_processor():
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor, DevicePrefetcher
    exp = DeviceImageProcessor(size=R.SIZE, dtype=torch.bfloat16)(images=SRC)["pixel_values"].clone()
    labels, boxes = _targets()
    n = 0
    for img, lab, box, _ in DevicePrefetcher(_loader(2), "cuda", size=R.SIZE, augment=None):
        assert torch.equal(img, exp)
        assert all(torch.equal(b.cpu(), b0) for b, b0 in zip(box, boxes))          # targets untouched: still xywh pixels
        n += 1
    assert n == 2


def test_prefetcher_target_transform_runs_after_the_augmentation_and_float_inputs_are_refused():
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher
    seen = []

    def tt(lab, box, meta):
        seen.append(all(float(b.max()) <= 1.0 and b.dtype == torch.float32 for b in box))      # normalised xyxy already
        return lab, [b * 0.5 for b in box], meta

    by_hand = _augment()
    labels, boxes = _targets()
    _, ob, _ = by_hand.sample(R.SHAPES, [b.numpy() for b in boxes], [l.numpy() for l in labels], 0, 0)
    for img, lab, box, meta in DevicePrefetcher(_loader(1), "cuda", size=R.SIZE, augment=_augment(), target_transform=tt, threaded=False):
        assert all(np.array_equal(b.cpu().numpy(), o * np.float32(0.5)) for b, o in zip(box, ob))
    assert seen == [True]

    def dense():
        yield torch.zeros(3, 3, R.SIZE, R.SIZE), labels, boxes
    with pytest.raises(ValueError, match="uint8"):
        next(iter(DevicePrefetcher(dense(), "cuda", size=R.SIZE, augment=_augment(), threaded=False)))
    with pytest.raises(ValueError, match="size"):
        DevicePrefetcher(_loader(1), "cuda", size=96, augment=_augment())


def test_train_step_from_an_augmented_batch():
    """One tiny-config train step fed by the augmenting prefetcher: every image has a target, the four losses are finite, the parameters move."""
    from owl_vit_object_detection_amd import weights
    from owl_vit_object_detection_amd.config import get_config
    from owl_vit_object_detection_amd.losses import PushPullLoss
    from owl_vit_object_detection_amd.models import OwlViT
    from owl_vit_object_detection_amd.optim import FusedAdamW
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher, TrainAugment
    cfg = get_config("tiny")
    S = cfg.image_size
    aug = TrainAugment(S, mosaic=(1, 2, 3), seed=2)
    model = OwlViT(cfg, weights.make_weights(cfg), "cuda")
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1)
    before = model.flat_param.detach().clone()
    for img, lab, box, _ in DevicePrefetcher(_loader(1), "cuda", size=S, augment=aug):
        assert tuple(img.shape) == (len(SRC), 3, S, S) and img.dtype == torch.bfloat16
        assert all(len(b) >= 1 and len(b) == len(l) for b, l in zip(box, lab))
        assert all(int(l.max()) < cfg.n_classes for l in lab)
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        losses = crit(ps, lab, pb, box)
        (losses["loss_ce"] + losses["loss_bg"] + losses["loss_bbox"] + losses["loss_giou"]).backward()
        opt.step()
        vals = torch.stack([losses[k].detach() for k in ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")]).cpu()
        assert torch.isfinite(vals).all(), vals
    torch.cuda.synchronize()
    assert aug.fallbacks == 0 and float((model.flat_param.detach() - before).abs().max()) > 0
