"""-m gpu: the two streams of the frozen-prefix activation cache (csrc/prefix_cache.hip) against torch indexing, bit for bit.

owl_prefix_emit forms `(xs + d1) + d2` with plain f32 adds in that order -- the expected value is formed the same way in torch f32 -- and writes it to each
image's destination block and, where the image has one, its slot; owl_prefix_gather copies slots to destination blocks.  Shapes: Tp = 40 rows (the `tiny`
configs') of D = 128 / 768 / 1024; n = 1, 5 and 70 images, 70 being more than the 64 one launch takes.  Every buffer starts at a sentinel, so a block
nobody names must come back untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from owl_vit_object_detection_amd import ops  # noqa: E402

DEV = "cuda"
TP = 40
SENTINEL = -777.25


def _operands(n, D, n_delta, seed):
    g = torch.Generator().manual_seed(seed)
    E = TP * D
    xs = torch.randn(n, E, generator=g).to(DEV)
    # bf16 branch outputs two to three binades below xs: every add rounds
    d = [(torch.randn(n, E, generator=g) * s).to(torch.bfloat16).to(DEV) for s in (0.37, 0.11)][:n_delta]
    return xs, (d + [None, None])[:2]


def _expected(xs, d1, d2):
    s = xs
    if d1 is not None:
        s = s + d1.float()
    if d2 is not None:
        s = s + d2.float()          # (xs + d1) + d2, in that order
    return s


@pytest.mark.parametrize("D", [128, 768, 1024])
@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("n_delta", [0, 1, 2])
def test_emit_is_torch_indexing_bit_for_bit(D, n, n_delta):
    E = TP * D
    xs, (d1, d2) = _operands(n, D, n_delta, seed=100 * n + n_delta)
    B = n + 3                                                  # the full batch has positions no fresh image goes to
    g = torch.Generator().manual_seed(n)
    pos = torch.randperm(B, generator=g)[:n].tolist()          # destinations out of order
    dst = torch.full((B, E), SENTINEL, device=DEV)
    # slots: out of order, in two slabs, and every third image without one
    slabs = [torch.full((n // 2 + 2, E), SENTINEL, device=DEV) for _ in range(2)]
    order = torch.randperm(n, generator=g).tolist()
    slot_of = [None if j % 3 == 2 else (order[j] % 2, order[j] // 2) for j in range(n)]
    ops.prefix_emit(xs, d1, d2, n, E, [dst[p].data_ptr() for p in pos], [0 if s is None else slabs[s[0]][s[1]].data_ptr() for s in slot_of])
    torch.cuda.synchronize()
    want = _expected(xs, d1, d2)
    want_dst = torch.full((B, E), SENTINEL, device=DEV)
    want_dst[pos] = want
    assert torch.equal(dst, want_dst)
    want_slabs = [torch.full_like(s, SENTINEL) for s in slabs]
    for j, s in enumerate(slot_of):
        if s is not None:
            want_slabs[s[0]][s[1]] = want[j]
    assert all(torch.equal(a, b) for a, b in zip(slabs, want_slabs))
    assert n < 3 or any(s is None for s in slot_of)


@pytest.mark.parametrize("D", [128, 768, 1024])
@pytest.mark.parametrize("n", [1, 5, 70])
def test_gather_is_torch_indexing_bit_for_bit(D, n):
    E = TP * D
    g = torch.Generator().manual_seed(7 * n + D)
    slabs = [torch.randn(n // 2 + 1, E, generator=g).to(DEV) for _ in range(2)]
    B = n + 4
    pos = torch.randperm(B, generator=g)[:n].tolist()
    pick = [(int(a) % 2, int(b) % (n // 2 + 1)) for a, b in zip(torch.randint(0, 2, (n,), generator=g), torch.randint(0, n, (n,), generator=g))]
    if n > 1:
        pick[-1] = pick[0]                                     # the same slot gathered to two positions
    dst = torch.full((B, E), SENTINEL, device=DEV)
    ops.prefix_gather(n, E, [slabs[a][b].data_ptr() for a, b in pick], [dst[p].data_ptr() for p in pos])
    torch.cuda.synchronize()
    want = torch.full((B, E), SENTINEL, device=DEV)
    for p, (a, b) in zip(pos, pick):
        want[p] = slabs[a][b]
    assert torch.equal(dst, want)                              # rows no image names keep the sentinel
    assert int((want[:, 0] == SENTINEL).sum()) == B - n


def test_emit_refuses_a_destination_inside_the_compacted_source():
    """In the no-grad forward the compacted source and the batch's residual stream are the same buffer: a workgroup writing position p could overwrite
    another image's unread source, so the entry point refuses the overlap instead of launching."""
    from owl_vit_object_detection_amd import _lib
    E = TP * 128
    xs = torch.zeros(3, E, device=DEV)
    with pytest.raises(_lib.OwlLibError, match="overlaps"):
        ops.prefix_emit(xs, None, None, 2, E, [xs[2].data_ptr(), xs[1].data_ptr()], [0, 0])
    spare = torch.empty(E, device=DEV)
    ops.prefix_emit(xs, None, None, 2, E, [xs[2].data_ptr(), spare.data_ptr()], [0, 0])          # block 2 lies past the n = 2 source blocks
    torch.cuda.synchronize()
