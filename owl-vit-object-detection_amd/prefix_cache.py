"""Frozen-prefix activation cache: the residual stream at the entry of the first non-frozen consumer, kept per image on the device.

Under a freeze rule the patch embedding, `pre_layernorm` and the encoder layers below the first one the backward crosses never change during a run, so the
f32 residual stream their last layer hands on -- `(xs + delta1) + delta2`, the value the next LayerNorm forms (models.OwlViT._encoder_layer) -- depends on the
pixels alone.  `model(image, image_ids=ids)` keeps it per id in device slabs and, for ids already kept, runs none of those layers.

This module is the host side: which id lives in which slot (`plan`, pure Python), the slabs (allocated lazily, so an unused budget costs nothing) and the
two launches (ops.prefix_emit / ops.prefix_gather, csrc/prefix_cache.hip).  Rules: first come, first kept until the budget is full; no eviction (an
epoch-shuffled loader gains nothing from LRU); an id that occurs twice in a batch is computed once and stored once.
"""
from collections import namedtuple

import torch

from . import ops

DEFAULT_MAX_BYTES = 32 << 30         # of the card's 288 GB: 4 800 images of B/16 at 768 x 768 (7.1 MB each) -- the reference's 2 500 + 100 fit
SLAB_BYTES = 256 << 20               # slots are carved out of slabs of about this size (at least one slot each)

# hit_pos / hit_slots: batch positions served from a slot.  miss_pos / miss_ids: positions (ascending) and ids of the images to compute, each id once;
# miss_slots: the slot each of them is admitted to, -1 = refused (budget full).  dup_pos / dup_src: later positions of an id the batch already computes,
# and the index into miss_pos of that first occurrence.
Plan = namedtuple("Plan", "hit_pos hit_slots miss_pos miss_ids miss_slots dup_pos dup_src")


def _id_list(ids):
    """-> list of Python ints.  Sequences and CPU tensors are taken; a device tensor is refused (reading it would be a hidden sync)."""
    if getattr(ids, "is_cuda", False):
        raise TypeError("image_ids must be a sequence or a CPU tensor of integers, got a device tensor: reading it would synchronise the stream "
                        "(pass the loader's indices as they come, before any .to(device))")
    if torch.is_tensor(ids):
        if ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.dim() != 1:
            raise TypeError(f"image_ids must be a 1-D integer tensor, got {tuple(ids.shape)} {ids.dtype}")
        return [int(v) for v in ids.tolist()]
    out = []
    for v in ids:
        if isinstance(v, bool) or not hasattr(v, "__index__"):
            raise TypeError(f"image_ids must be integers, got {type(v).__name__}")
        out.append(int(v.__index__()))
    return out


class PrefixCache:
    """Slots of `block_elems` f32 elements, one per kept image id.  `key`: what the kept values depend on besides the pixels (the model's config); the
    owner compares it.  capacity = min(max_bytes // bytes per slot, max_images)."""

    def __init__(self, block_elems: int, max_bytes: int = DEFAULT_MAX_BYTES, max_images=None, device="cuda", key=None):
        if block_elems <= 0 or block_elems % 8:
            raise ValueError(f"PrefixCache: block_elems = {block_elems} must be a positive multiple of 8")
        if max_bytes is None:
            max_bytes = DEFAULT_MAX_BYTES
        if max_bytes < 0 or (max_images is not None and max_images < 0):
            raise ValueError("PrefixCache: max_bytes and max_images must not be negative")
        self.block_elems, self.block_bytes = int(block_elems), 4 * int(block_elems)
        self.max_bytes, self.max_images = int(max_bytes), None if max_images is None else int(max_images)
        self.capacity = self.max_bytes // self.block_bytes
        if self.max_images is not None:
            self.capacity = min(self.capacity, self.max_images)
        self.slab_slots = max(1, SLAB_BYTES // self.block_bytes)
        self.device, self.key = torch.device(device), key
        self._slot_of, self._slabs = {}, []
        self._counts = dict(hits=0, misses=0, admitted=0, refused=0, duplicates=0)

    # -- bookkeeping (host only) ---------------------------------------------------------------------------
    def __len__(self):
        return len(self._slot_of)

    def contains(self, ids):
        """[id is kept, ...] -- the hook for a loader that wants to skip decoding images the model will not read."""
        return [i in self._slot_of for i in _id_list(ids)]

    @property
    def nbytes(self) -> int:
        """Device bytes the slabs hold now (never above max_bytes)."""
        return sum(s.numel() * 4 for s in self._slabs)

    @property
    def stats(self):
        return dict(self._counts, slots=len(self._slot_of), bytes=self.nbytes)

    def clear(self):
        """Forget every id and release the slabs (the counters stay: they describe the run)."""
        self._slot_of.clear()
        self._slabs = []

    def plan(self, ids) -> Plan:
        """What a batch with these ids does, decided on the host alone (no device call, nothing changes): hits read their slots, every other id is
        computed once, the first `capacity - len(self)` of them in batch order get the next free slots, later occurrences of an id copy its first one."""
        ids = _id_list(ids)
        hit_pos, hit_slots, miss_pos, miss_ids, miss_slots, dup_pos, dup_src = [], [], [], [], [], [], []
        first, nxt = {}, len(self._slot_of)
        for pos, i in enumerate(ids):
            if i in self._slot_of:
                hit_pos.append(pos); hit_slots.append(self._slot_of[i])
            elif i in first:
                dup_pos.append(pos); dup_src.append(first[i])
            else:
                first[i] = len(miss_pos)
                miss_pos.append(pos); miss_ids.append(i)
                if nxt < self.capacity:
                    miss_slots.append(nxt); nxt += 1
                else:
                    miss_slots.append(-1)
        return Plan(hit_pos, hit_slots, miss_pos, miss_ids, miss_slots, dup_pos, dup_src)

    def commit(self, plan: Plan):
        """Record what `plan` admitted (its slots are written, or about to be, on the stream every later read is ordered behind) and count."""
        for i, s in zip(plan.miss_ids, plan.miss_slots):
            if s >= 0:
                if s != len(self._slot_of) or i in self._slot_of:
                    raise RuntimeError("PrefixCache.commit: the plan was made for another state of the cache (plan and commit go together, one batch at a time)")
                self._slot_of[i] = s
        c = self._counts
        c["hits"] += len(plan.hit_pos); c["misses"] += len(plan.miss_pos); c["duplicates"] += len(plan.dup_pos)
        c["admitted"] += sum(1 for s in plan.miss_slots if s >= 0); c["refused"] += sum(1 for s in plan.miss_slots if s < 0)

    # -- slabs ------------------------------------------------------------------------------------------------
    def _slab_len(self, k: int) -> int:
        return min(self.slab_slots, self.capacity - k * self.slab_slots)

    def slot_addr(self, slot: int) -> int:
        """Device address of a slot; the slab that holds it is allocated on first use (on the current stream)."""
        if not 0 <= slot < self.capacity:
            raise IndexError(f"PrefixCache: slot {slot} outside the capacity of {self.capacity}")
        k, j = divmod(slot, self.slab_slots)
        while len(self._slabs) <= k:
            self._slabs.append(torch.empty(self._slab_len(len(self._slabs)) * self.block_elems, dtype=torch.float32, device=self.device))
        return self._slabs[k].data_ptr() + j * self.block_bytes

    def slot_view(self, slot: int) -> torch.Tensor:
        """The slot as a tensor [block_elems] (tests, tools)."""
        k, j = divmod(slot, self.slab_slots)
        self.slot_addr(slot)
        return self._slabs[k][j * self.block_elems:(j + 1) * self.block_elems]

    # -- the two launches ---------------------------------------------------------------------------------------
    def fill(self, plan: Plan, dst: torch.Tensor, xs=None, delta1=None, delta2=None):
        """Bring the batch's boundary state into `dst` ([>= B, block] f32 rows, position p at block p) on the current stream: the computed images -- blocks
        0 .. len(miss_pos) - 1 of xs / delta1 / delta2, in miss order -- are summed into their positions and admitted slots (one emit), then hits and
        repeated ids are copied in (one gather, behind the emit).  `dst` must not overlap xs."""
        E, base = self.block_elems, dst.data_ptr()
        m = len(plan.miss_pos)
        if m:
            ops.prefix_emit(xs, delta1, delta2, m, E, [base + p * self.block_bytes for p in plan.miss_pos],
                            [self.slot_addr(s) if s >= 0 else 0 for s in plan.miss_slots])
        src = [self.slot_addr(s) for s in plan.hit_slots] + [base + plan.miss_pos[j] * self.block_bytes for j in plan.dup_src]
        pos = list(plan.hit_pos) + list(plan.dup_pos)
        if pos:
            ops.prefix_gather(len(pos), E, src, [base + p * self.block_bytes for p in pos])
        self.commit(plan)
