"""Host staging of image crops: a thread pool cuts the crops of a batch STRAIGHT INTO pinned host buffers, chunk by chunk,
and the consumer uploads a chunk as soon as its workers are done -- so the ViT of chunk k is queued while chunk k+1 is
still being cut, and a serving loop can have batch k+1 cut under batch k's GPU time.

Ownership of a pinned buffer is a property of objects, not a convention:
  * ``PinnedRing.take`` hands a buffer out as a ``Lease``; the lease gives it back exactly once, by ``upload`` (reusable
    when the copy's event has passed) or by ``release``.  Either is a no-op on a lease that has given its buffer back,
    and a lease never touches a slot that has since been handed to someone else (the slot's generation).
  * a ``StagedBatch`` owns the leases of the chunks nobody has taken yet; ``next_chunk`` transfers one to the caller,
    ``drain`` (== leaving the ``with`` block) gives back the rest once their workers have stopped writing.
Host only: no kernels, no model; the two device-touching operations of the ring can be replaced (tests without a GPU).
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image


def plan_chunks(counts: Sequence[int], chunk_crops: int) -> List[Tuple[int, int, int]]:
    """[(i0, i1, crops)]: consecutive images whose crop counts total <= ``chunk_crops`` (at least one image per chunk)."""
    chunks, i0, n = [], 0, len(counts)
    while i0 < n:
        i1, tot = i0, 0
        while i1 < n and (i1 == i0 or tot + counts[i1] <= max(chunk_crops, 1)):
            tot += counts[i1]
            i1 += 1
        chunks.append((i0, i1, tot))
        i0 = i1
    return chunks


def crop_workers(affinity_cpus: int, total_cpus: int, ranks_here: int) -> int:
    """Threads of the crop pool.  One process per GPU: the ranks of a node share its cores (8 ranks x 32 workers + prefetch
    workers would oversubscribe a 256-thread host)."""
    n = affinity_cpus
    if ranks_here > 1 and n * ranks_here <= total_cpus + ranks_here:
        share = n  # the affinity mask already IS this rank's share (dist.bind_rank_cpus): do not divide twice
    else:
        share = n // ranks_here
    return max(1, min(32, share - 2 if ranks_here > 1 else n))


def _pinned_bytes(nbytes: int) -> torch.Tensor:
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


def _record_event(device):
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    return ev


class _Slot:
    __slots__ = ("buf", "event", "busy", "gen")

    def __init__(self, buf: torch.Tensor):
        self.buf, self.event, self.busy, self.gen = buf, None, False, 0


class PinnedRing:
    """PINNED staging for the uint8 crops (a pageable source makes the runtime bounce the copy through its own small pinned
    buffers, synchronously: ~2x the time, and the host cannot queue the ViT launches behind it).  A small set of buffers
    rotates; a buffer is handed out again only after the copy that read it has completed (its event)."""

    def __init__(self, alloc: Callable[[int], torch.Tensor] = _pinned_bytes, record_event: Callable = _record_event):
        self.slots: List[_Slot] = []
        self._alloc, self._record_event = alloc, record_event

    def take(self, nbytes: int) -> "Lease":
        nbytes = int(nbytes)
        slot = next((s for s in self.slots if not s.busy and s.buf.numel() >= nbytes), None)
        if slot is None:
            with torch.inference_mode(False):
                slot = _Slot(self._alloc(max(nbytes, 1 << 20)))
            self.slots.append(slot)
        if slot.event is not None:
            slot.event.synchronize()
            slot.event = None
        slot.busy = True
        slot.gen += 1
        return Lease(self, slot, nbytes)


class Lease:
    """One hand-out of a ring buffer.  ``with lease:`` releases on exit, i.e. gives the buffer back unless ``upload`` has."""

    __slots__ = ("_ring", "_slot", "_gen", "_nbytes", "_shape")

    def __init__(self, ring: PinnedRing, slot: _Slot, nbytes: int):
        self._ring, self._slot, self._gen, self._nbytes, self._shape = ring, slot, slot.gen, nbytes, (nbytes,)

    @property
    def held(self) -> bool:
        return self._slot.busy and self._slot.gen == self._gen

    def array(self, shape) -> np.ndarray:
        """The host buffer as a uint8 array of ``shape`` (which ``upload`` then gives the device tensor)."""
        self._shape = tuple(int(s) for s in shape)
        return self._slot.buf[: self._nbytes].numpy().reshape(self._shape)

    def upload(self, device) -> torch.Tensor:
        """Non-blocking copy to ``device`` on the current stream; the slot is reusable once the copy's event has passed
        (checked when it is handed out again)."""
        if not self.held:
            raise RuntimeError("upload from a pinned buffer that this lease has given back")
        dev = self._slot.buf[: self._nbytes].view(self._shape).to(device, non_blocking=True)
        self._slot.event = self._ring._record_event(device)
        self._slot.busy = False
        return dev

    def release(self) -> None:
        if self.held:
            self._slot.busy = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()


class StagedBatch:
    """The chunks of one batch whose buffers nobody has taken yet: [(lease, futures, i0, i1)], in order."""

    __slots__ = ("chunks",)

    def __init__(self):
        self.chunks: list = []

    def next_chunk(self):
        """(results of the first chunk's workers, its lease): the lease is the caller's from here.  A worker's exception
        is raised with the chunk still owned by the batch."""
        part = [f.result() for f in self.chunks[0][1]]
        return part, self.chunks.pop(0)[0]

    def wait(self) -> None:
        for _, futs, _, _ in self.chunks:
            for f in futs:
                f.result()

    def drain(self) -> None:
        """Give back the buffers still owned (idempotent)."""
        while self.chunks:
            lease, futs, _, _ = self.chunks.pop(0)
            for f in futs:
                try:
                    f.result()  # the worker must be done with the buffer before it is handed out again
                except Exception:
                    pass  # (a failed crop was / will be reported by the consumer; here only the buffer matters)
            lease.release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.drain()


def upload_unique(ring: PinnedRing, part, crop_shape, device):
    """Upload a chunk's crops (``part``: its workers' results, still in the chunk's buffer: the caller holds that lease)
    with byte-identical crops of an image sent once -> (device crops, expand): ``feats[expand]`` are the features of the
    chunk's crops when ``len(expand) != len(device crops)``.

    An image that is no larger than one crop has tiling (1, 1) and its single local crop holds the same pixels as the
    global crop (image_crops.py:124-167: both are the image resized to crop_size).  The encoder maps equal inputs to
    equal outputs whatever else is in the launch, so such a crop is encoded once and its features are used for both
    positions."""
    uniq, expand = [], []
    for c, tiling in part:
        if tiling == (1, 1) and c.shape[0] == 2 and np.array_equal(c[0], c[1]):
            expand += [len(uniq), len(uniq)]
            uniq.append(c[:1])
        else:
            expand += list(range(len(uniq), len(uniq) + c.shape[0]))
            uniq.extend(c[k : k + 1] for k in range(c.shape[0]))
    shape = (len(uniq),) + tuple(crop_shape)
    with ring.take(int(np.prod(shape))) as second:  # the unique crops' buffer: the upload takes it over, an error gives it back
        np.concatenate(uniq, axis=0, out=second.array(shape))
        return second.upload(device), expand


class CropStager:
    """The ring, the two thread pools and the table of batches staged ahead.  ``count_crops(image)`` -> crops the image
    is cut into; ``crop_into(image, out)`` cuts them into ``out`` [n, *crop_shape] uint8 and returns (crops, tiling);
    ``pool_workers()`` -> threads of the crop pool, asked when the pool is first needed."""

    def __init__(self, count_crops: Callable, crop_into: Callable, crop_shape: Tuple[int, ...], pool_workers: Callable[[], int],
                 ring: Optional[PinnedRing] = None):
        self.count_crops, self.crop_into, self.crop_shape, self._pool_workers = count_crops, crop_into, tuple(crop_shape), pool_workers
        self.ring = ring if ring is not None else PinnedRing()
        self._pool = self._prefetch_pool = None
        self.prefetched: Dict[tuple, Tuple[list, StagedBatch]] = {}  # image identities -> (the images, kept alive; batch)

    def stage(self, images: Sequence[Image.Image], chunk_crops: int, pool=None) -> StagedBatch:
        """Queue the host tiling of a batch on the thread pool, chunk by chunk, each image cutting its crops into its
        slice of a pinned staging buffer (the tiling, hence every image's crop count and offset, follows from its size
        alone: no concatenation pass over the crop bytes on the host)."""
        if pool is None:
            if self._pool is None:
                self._pool = ThreadPoolExecutor(max_workers=self._pool_workers())
            pool = self._pool
        counts = [self.count_crops(im) for im in images]
        batch = StagedBatch()
        try:
            for i0, i1, tot in plan_chunks(counts, chunk_crops):  # all host work is queued up front; the GPU side follows chunk by chunk
                shape = (tot,) + self.crop_shape
                lease = self.ring.take(int(np.prod(shape)))
                futs: list = []
                batch.chunks.append((lease, futs, i0, i1))
                host, off = lease.array(shape), 0
                for i in range(i0, i1):
                    futs.append(pool.submit(self.crop_into, images[i], host[off : off + counts[i]]))
                    off += counts[i]
        except BaseException:
            batch.drain()
            raise
        return batch

    def prefetch(self, images: Sequence[Image.Image], chunk_crops: int, workers: int = 4) -> None:
        """Stage a batch now for a later ``take`` of exactly these image objects.  At most two batches are held (the
        one about to run + one ahead); the oldest is drained to make room."""
        images = list(images)  # (kept alive with the entry: the key is made of object identities)
        key = tuple(id(im) for im in images)
        if key in self.prefetched:
            return
        while len(self.prefetched) >= 2:
            self.discard(next(iter(self.prefetched)))
        # a FEW background workers: the step that is running needs the host for its own launches, and the tiling of one
        # batch (tens of ms of CPU per large image) has a whole step's GPU time to finish
        if self._prefetch_pool is None:
            self._prefetch_pool = ThreadPoolExecutor(max_workers=max(1, int(workers)))
        self.prefetched[key] = (images, self.stage(images, chunk_crops, self._prefetch_pool))

    def take(self, images: Sequence[Image.Image], chunk_crops: int) -> StagedBatch:
        """The batch staged ahead for exactly these image objects, else one staged now.  (An entry leaves the table only
        to be used: popped and dropped it would leak its buffers.)"""
        pre = self.prefetched.pop(tuple(id(im) for im in images), None)
        return pre[1] if pre is not None else self.stage(images, chunk_crops)

    def wait_prefetched(self) -> None:
        for _, batch in self.prefetched.values():
            batch.wait()

    def discard(self, key=None) -> None:
        """Drop batches staged ahead that were never used (waits for their workers, gives their buffers back)."""
        for k in [key] if key is not None else list(self.prefetched):
            self.prefetched.pop(k)[1].drain()
