"""Colour jitter on the device: `owl_preprocess_u8_tiles_color` against the numpy restatement of Pillow's resize / flip / ImageEnhance / paste
(tests/color_reference.py, pinned to PIL by tests/test_color_reference.py), bit for bit, f32 and bf16 -- on 24-pixel canvases at mosaic grids 1, 2, 3 and
on 330-pixel ones (a cell two workgroups wide, a row count that is no multiple of the four-row unit) -- its bitwise properties, and the same through
`DevicePrefetcher(augment=TrainAugment(..., color=ColorJitter(...)))`.  tests/test_color_reference.py shows that each of seven plausible kernel errors
changes at least one of the cases compared here."""
import numpy as np
import pytest
import torch

from tests import augment_reference as R
from tests import color_reference as C

pytestmark = pytest.mark.gpu

SRC = C.sources()
CASES = C.cases()
_REF = {}


def _ref(name):
    """f32 [n,3,S,S] reference pixel_values of a case, computed once."""
    if name not in _REF:
        tiles, color, n_out, size = CASES[name]
        _REF[name] = torch.from_numpy(C.pixel_values(C.render_color(SRC, tiles, color, n_out, size)))
    return _REF[name]


def _ptiles(tiles):
    from owl_vit_object_detection_amd.preprocess import Tile
    return [Tile(*t) for t in tiles]


def _ip(size, dtype=torch.float32):
    from owl_vit_object_detection_amd.preprocess import DeviceImageProcessor
    return DeviceImageProcessor(size=size, dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(CASES))
def test_colour_tiles_equal_the_restatement(name, dtype):
    tiles, color, n_out, size = CASES[name]
    got = _ip(size, dtype).tiles(SRC, _ptiles(tiles), n_out, color=color)
    assert got.dtype == dtype and tuple(got.shape) == (n_out, 3, size, size)
    assert torch.equal(got.cpu(), _ref(name).to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["mixed", "big"])
def test_all_ones_is_the_plain_tile_path(name, dtype):
    tiles, _, n_out, size = CASES[name]
    ip = _ip(size, dtype)
    plain = ip.tiles(SRC, _ptiles(tiles), n_out).clone()
    assert torch.equal(ip.tiles(SRC, _ptiles(tiles), n_out, color=np.ones((len(tiles), 4), dtype=np.float32)), plain)
    assert torch.equal(ip.tiles(SRC, _ptiles(tiles), n_out), plain)                         # and the plain path after a colour launch


def test_tile_order_does_not_change_the_bits_and_two_runs_are_equal():
    for name in ("mixed", "big"):
        tiles, color, n_out, size = CASES[name]
        ip = _ip(size)
        a = ip.tiles(SRC, _ptiles(tiles), n_out, color=color).cpu()
        b = ip.tiles(SRC, _ptiles(tiles), n_out, color=color).cpu()
        assert torch.equal(a, b) and torch.equal(a, _ref(name))
        perm = np.random.default_rng(0).permutation(len(tiles))
        assert not np.array_equal(perm, np.arange(len(tiles)))
        got = ip.tiles(SRC, [_ptiles(tiles)[i] for i in perm], n_out, color=color[perm])
        assert torch.equal(got.cpu(), _ref(name))
        got = ip.tiles(SRC, _ptiles(tiles)[::-1], n_out, color=color[::-1])
        assert torch.equal(got.cpu(), _ref(name))


def test_a_cell_does_not_depend_on_its_neighbours_factors():
    tiles, color, n_out, size = CASES["mixed"]
    ip = _ip(size)
    base = ip.tiles(SRC, _ptiles(tiles), n_out, color=color).cpu()
    k = 7                                                        # a cell of the 3 x 3 canvas
    t = tiles[k]
    other = np.array(color, copy=True)
    rng = np.random.default_rng(8)
    for j in range(len(tiles)):
        if j != k:
            other[j] = (*rng.uniform(0.0, 2.0, 3), (other[j, 3] + 1) % 6)
    got = ip.tiles(SRC, _ptiles(tiles), n_out, color=other).cpu()
    cell = (t.b, slice(None), slice(t.y0, t.y0 + t.ch), slice(t.x0, t.x0 + t.cw))
    assert torch.equal(got[cell], base[cell]) and not torch.equal(got, base)
    assert torch.equal(got, torch.from_numpy(C.pixel_values(C.render_color(SRC, tiles, other, n_out, size))))


def test_bad_colour_rows_raise_before_the_launch():
    tiles, color, n_out, size = CASES["mixed"]
    ip = _ip(size)
    bad = np.array(color, copy=True)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="color"):
        ip.tiles(SRC, _ptiles(tiles), n_out, color=bad)
    with pytest.raises(ValueError, match="shape"):
        ip.tiles(SRC, _ptiles(tiles), n_out, color=color[:-1])


# ---- through the prefetcher ------------------------------------------------------------------------------------------------------------------------
TEX = SRC[:3]                                                    # the loader's batch: the three textured sources


def _targets():
    boxes = [torch.tensor([[W / 4, H / 4, W / 2, H / 2]], dtype=torch.float32) for H, W in R.SHAPES]      # COCO xywh pixels: the central quarter
    labels = [torch.tensor([k]) for k in range(len(R.SHAPES))]
    return labels, boxes


def _loader(n_batches):
    labels, boxes = _targets()
    for i in range(n_batches):
        yield [torch.from_numpy(im) for im in TEX], labels, boxes, {"batch": i}


def _augment(color=True, size=R.SIZE, seed=21):
    from owl_vit_object_detection_amd.preprocess import ColorJitter, TrainAugment
    return TrainAugment(size, mosaic=(1, 2, 3), seed=seed, color=ColorJitter(0.4, 0.4, 0.4, gray=0.2) if color else None)


@pytest.mark.parametrize("threaded", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_prefetcher_batch_is_the_sampler_plus_the_restatement(dtype, threaded):
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher
    pf = DevicePrefetcher(_loader(3), "cuda", size=R.SIZE, dtype=dtype, augment=_augment(), threaded=threaded)
    pf.set_epoch(4)
    by_hand = _augment()
    labels, boxes = _targets()
    grids, n, jittered = set(), 0, 0
    for i, (img, lab, box, meta) in enumerate(pf):
        tiles, ob, ol = by_hand.sample(R.SHAPES, [b.numpy() for b in boxes], [l.numpy() for l in labels], 4, i)
        color = by_hand.color.sample(len(tiles), (21, 0, 4, i))
        jittered += int((color[:, :3] != 1).any(axis=1).sum())
        grids |= {R.SIZE // t.cw for t in tiles}
        exp = torch.from_numpy(C.pixel_values(C.render_color(TEX, tiles, color, len(TEX), R.SIZE))).to(dtype)
        assert img.is_cuda and img.dtype == dtype and torch.equal(img.cpu(), exp)
        assert meta == {"batch": i}
        for j in range(len(TEX)):
            assert np.array_equal(box[j].cpu().numpy(), ob[j]) and np.array_equal(lab[j].cpu().numpy(), ol[j])
        n += 1
    assert n == 3 and len(grids) > 1 and jittered > 0


def test_prefetcher_same_seed_and_epoch_same_bits():
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher

    def run(epoch, threaded):
        pf = DevicePrefetcher(_loader(2), "cuda", size=R.SIZE, dtype=torch.float32, augment=_augment(), threaded=threaded)
        pf.set_epoch(epoch)
        return [img.cpu() for img, _, _, _ in pf]

    a, b, c = run(1, True), run(1, False), run(2, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not all(torch.equal(x, y) for x, y in zip(a, c))


def test_prefetcher_colour_off_is_todays_batch_and_targets_do_not_depend_on_colour():
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher

    def run(aug):
        pf = DevicePrefetcher(_loader(2), "cuda", size=R.SIZE, dtype=torch.bfloat16, augment=aug, threaded=False)
        pf.set_epoch(3)
        return [(img.cpu(), [b.cpu() for b in box], [l.cpu() for l in lab]) for img, lab, box, _ in pf]

    from owl_vit_object_detection_amd.preprocess import TrainAugment
    off, on, before = run(_augment(color=False)), run(_augment()), run(TrainAugment(R.SIZE, mosaic=(1, 2, 3), seed=21))
    labels, boxes = _targets()
    plain = _augment(color=False)
    for i, ((io, bo, lo), (ic, bc, lc), (ib, _, _)) in enumerate(zip(off, on, before)):
        tiles, _, _ = plain.sample(R.SHAPES, [b.numpy() for b in boxes], [l.numpy() for l in labels], 3, i)
        exp = torch.from_numpy(R.pixel_values(R.render(TEX, tiles, len(TEX), R.SIZE))).to(torch.bfloat16)
        assert torch.equal(io, exp) and torch.equal(io, ib)                                # color=None: the augmented batch as it was
        assert not torch.equal(io, ic)                                                      # colour on: other pixels ...
        assert all(torch.equal(x, y) for x, y in zip(bo, bc)) and all(torch.equal(x, y) for x, y in zip(lo, lc))     # ... the same targets


def test_train_step_from_a_jittered_batch():
    """One tiny-config train step fed by the jittering prefetcher: the four losses are finite, the parameters move."""
    from owl_vit_object_detection_amd import weights
    from owl_vit_object_detection_amd.config import get_config
    from owl_vit_object_detection_amd.losses import PushPullLoss
    from owl_vit_object_detection_amd.models import OwlViT
    from owl_vit_object_detection_amd.optim import FusedAdamW
    from owl_vit_object_detection_amd.preprocess import DevicePrefetcher
    cfg = get_config("tiny")
    S = cfg.image_size
    aug = _augment(size=S, seed=2)
    model = OwlViT(cfg, weights.make_weights(cfg), "cuda")
    crit = PushPullLoss(cfg.n_classes, None)
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.1)
    before = model.flat_param.detach().clone()
    for img, lab, box, _ in DevicePrefetcher(_loader(1), "cuda", size=S, augment=aug):
        assert tuple(img.shape) == (len(TEX), 3, S, S) and img.dtype == torch.bfloat16
        opt.zero_grad()
        pb, _, ps, _ = model(img)
        losses = crit(ps, lab, pb, box)
        (losses["loss_ce"] + losses["loss_bg"] + losses["loss_bbox"] + losses["loss_giou"]).backward()
        opt.step()
        vals = torch.stack([losses[k].detach() for k in ("loss_ce", "loss_bg", "loss_bbox", "loss_giou")]).cpu()
        assert torch.isfinite(vals).all(), vals
    torch.cuda.synchronize()
    assert float((model.flat_param.detach() - before).abs().max()) > 0
