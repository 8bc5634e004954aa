"""Crop staging without a GPU (moondream_amd/crop_staging.py): the chunk plan, the pool size, the ring's hand-out policy, and
-- the point of the module -- that every pinned buffer comes back exactly once whatever path a batch takes.  The ring gets a
pageable allocator and an event that only counts; crops are tiny and the crop function writes the image's one pixel value."""
import numpy as np
import pytest
import torch
from PIL import Image

from moondream_amd.crop_staging import CropStager, Lease, PinnedRing, crop_workers, plan_chunks, upload_unique

CROP = (4, 4, 3)
CROP_BYTES = 4 * 4 * 3


class FakeEvent:
    def __init__(self):
        self.syncs = 0

    def synchronize(self):
        self.syncs += 1


class Fakes:
    """A ring on pageable memory + the count of what it hands out and gets back: ``taken`` / ``returned`` hold one
    (slot, generation) per lease, ``returned`` one per call of upload / release that really gave a buffer back."""

    def __init__(self, monkeypatch):
        self.allocs, self.events, self.taken, self.returned, self.fail_alloc = [], [], [], [], False
        self.ring = PinnedRing(alloc=self._alloc, record_event=self._record)
        take = self.ring.take

        def counted_take(nbytes):
            lease = take(nbytes)
            self.taken.append((id(lease._slot), lease._gen))
            return lease

        self.ring.take = counted_take
        for name in ("upload", "release"):
            monkeypatch.setattr(Lease, name, self._counted(getattr(Lease, name)))

    def _alloc(self, nbytes):
        if self.fail_alloc:
            raise MemoryError("no pinned memory")
        self.allocs.append(nbytes)
        return torch.empty(nbytes, dtype=torch.uint8)

    def _record(self, device):
        self.events.append(FakeEvent())
        return self.events[-1]

    def _counted(self, method):
        def wrapper(lease, *args):
            held = lease.held
            try:
                return method(lease, *args)
            finally:
                if held and not lease.held:
                    self.returned.append((id(lease._slot), lease._gen))
        return wrapper

    def all_back_once(self):
        assert not any(s.busy for s in self.ring.slots)
        assert sorted(self.returned) == sorted(self.taken) and len(set(self.taken)) == len(self.taken)


@pytest.fixture
def fakes(monkeypatch):
    return Fakes(monkeypatch)


def image(value, crops=2, bad=False):
    im = Image.new("RGB", (3, 3), (value, value, value))
    im.info.update(crops=crops, bad=bad)
    return im


def count_crops(im):
    return im.info["crops"]


def crop_into(im, out):
    if im.info["bad"]:
        raise ValueError("bad image")
    out[:] = im.getpixel((0, 0))[0]
    return out, ((1, 1) if out.shape[0] == 2 else (1, out.shape[0] - 1))


def stager(fakes):
    return CropStager(count_crops, crop_into, CROP, lambda: 2, ring=fakes.ring)


# ------------------------------------------------------------------ pure decisions
def plan_chunks_before(counts, vit_chunk_crops):
    """The chunk loop as ``MoondreamModel._stage_crops`` had it, verbatim but for the names of its inputs."""
    n_img = len(counts)
    per_chunk = max(1, vit_chunk_crops // 2)
    chunks, i0 = [], 0
    while i0 < n_img:
        i1, tot = i0, 0
        while i1 < n_img and (i1 == i0 or (tot + counts[i1] <= max(vit_chunk_crops, 1) and i1 - i0 < per_chunk * 8)):
            tot += counts[i1]
            i1 += 1
        chunks.append((i0, i1, tot))
        i0 = i1
    return chunks


COUNT_LISTS = [[2] * 64, [13] * 32, [2, 13, 5, 2, 2, 10, 13], [13]]


@pytest.mark.parametrize("chunk_crops", [0, 1, 4, 32, 64])
@pytest.mark.parametrize("counts", COUNT_LISTS, ids=["2x64", "13x32", "mixed", "one13"])
def test_plan_chunks_equals_the_loop_it_replaces(counts, chunk_crops):
    plan = plan_chunks(counts, chunk_crops)
    assert plan == plan_chunks_before(counts, chunk_crops)
    assert [c[0] for c in plan] == [0] + [c[1] for c in plan[:-1]] and plan[-1][1] == len(counts)  # a partition, in order
    # The old loop also stopped a chunk at 8 * max(1, chunk_crops // 2) images.  With >= 2 crops per image (crop_count
    # never returns less) the crop budget stops it first: a chunk of more than one image holds <= chunk_crops // 2 of
    # them.  So that bound never decided anything and plan_chunks does not have it.
    assert all(i1 - i0 == 1 or i1 - i0 <= chunk_crops // 2 for i0, i1, _ in plan)
    assert all(i1 - i0 < 8 * max(1, chunk_crops // 2) for i0, i1, _ in plan)


@pytest.mark.parametrize("affinity, total, ranks, want", [(64, 64, 1, 32), (32, 256, 8, 30), (256, 256, 8, 30), (1, 1, 1, 1)])
def test_crop_workers(affinity, total, ranks, want):
    assert crop_workers(affinity, total, ranks) == want


# ------------------------------------------------------------------ ring and lease
def test_ring_takes_the_first_free_slot_that_fits_and_grows_by_at_least_1mib(fakes):
    ring = fakes.ring
    a = ring.take(100)
    assert fakes.allocs == [1 << 20]                    # max(nbytes, 1 MiB)
    b = ring.take((1 << 20) + 1)
    assert fakes.allocs == [1 << 20, (1 << 20) + 1]     # slot 0 is busy (and too small): a new buffer of nbytes
    c = ring.take(8)
    assert len(ring.slots) == 3
    a.release(), b.release(), c.release()
    assert ring.take(50)._slot is ring.slots[0]         # the first free one that fits, not the best fit
    assert ring.take((1 << 20) + 1)._slot is ring.slots[1]
    d = ring.take(1 << 20)
    assert d._slot is ring.slots[2] and len(fakes.allocs) == 3
    assert d.array((1 << 10, 1 << 10)).shape == (1 << 10, 1 << 10) and d.array((1 << 20,)).dtype == np.uint8


def test_slot_with_a_pending_upload_is_handed_out_after_one_synchronize(fakes):
    ring = fakes.ring
    a = ring.take(CROP_BYTES * 2)
    a.array((2,) + CROP)[:] = 7
    dev = a.upload("cpu")
    assert dev.shape == (2,) + CROP and int(dev.min()) == 7
    (ev,) = fakes.events
    assert ev.syncs == 0 and not ring.slots[0].busy and ring.slots[0].event is ev
    b = ring.take(10)
    assert b._slot is ring.slots[0] and ev.syncs == 1 and ring.slots[0].event is None
    b.release()
    ring.take(10)
    assert ev.syncs == 1 and len(ring.slots) == 1       # no event pending any more: nothing to wait for


def test_a_lease_gives_back_once_and_never_someone_elses_slot(fakes):
    ring = fakes.ring
    a = ring.take(10)
    a.upload("cpu")
    a.release()                                         # after upload(): a no-op (the pending event stays)
    assert ring.slots[0].event is fakes.events[0] and len(fakes.returned) == 1
    b = ring.take(10)                                   # the same slot, leased again
    assert b._slot is a._slot and b.held and not a.held
    a.release()                                         # stale: must leave b's slot busy
    assert ring.slots[0].busy and b.held
    with pytest.raises(RuntimeError):
        a.upload("cpu")
    b.release()
    b.release()                                         # a second release: a no-op
    c = ring.take(10)
    b.release()                                         # ... also once the slot is c's
    assert c.held and ring.slots[0].busy
    with c:
        pass
    fakes.all_back_once()
    assert len(fakes.taken) == 3


# ------------------------------------------------------------------ ownership of a batch's buffers
def consume(batch, ring, dedup=False):
    """What ``MoondreamModel._run_vision_encoder_batch`` does with a batch, minus the GPU."""
    got = []
    with batch:
        for _ in range(len(batch.chunks)):
            part, lease = batch.next_chunk()
            with lease:
                dev = upload_unique(ring, part, CROP, "cpu")[0] if dedup else lease.upload("cpu")
            got.append(dev)
    return got


def test_batch_fully_consumed(fakes):
    st = stager(fakes)
    images = [image(i + 1) for i in range(7)]
    batch = st.stage(images, 4)                         # 2 crops each, 4 per chunk: 4 chunks
    assert [(i0, i1) for _, _, i0, i1 in batch.chunks] == [(0, 2), (2, 4), (4, 6), (6, 7)]
    got = consume(batch, st.ring)
    assert [int(d[0, 0, 0, 0]) for d in got] == [1, 3, 5, 7] and [d.shape[0] for d in got] == [4, 4, 4, 2]
    assert not batch.chunks and len(fakes.events) == 4 and len(fakes.taken) == 4
    fakes.all_back_once()


def test_worker_that_raises(fakes):
    st = stager(fakes)
    images = [image(i + 1, bad=(i == 2)) for i in range(7)]
    batch = st.stage(images, 4)
    with pytest.raises(ValueError, match="bad image"):
        consume(batch, st.ring)
    assert len(fakes.events) == 1 and len(fakes.taken) == 4   # the first chunk went up; the drain gave the other three back
    fakes.all_back_once()
    assert [int(d[0, 0, 0, 0]) for d in consume(st.stage(images[:2], 4), st.ring)] == [1]  # the ring is whole


def test_drain_with_chunks_pending_and_again(fakes):
    st = stager(fakes)
    batch = st.stage([image(i + 1) for i in range(6)], 4)
    part, lease = batch.next_chunk()
    lease.upload("cpu")
    batch.drain()
    assert not batch.chunks
    fakes.all_back_once()
    batch.drain()
    lease.release()
    fakes.all_back_once()
    assert len(fakes.taken) == 3


def test_dedup_upload_sends_equal_crops_once(fakes):
    st = stager(fakes)
    (dev,) = consume(st.stage([image(1), image(2, crops=3)], 8), st.ring, dedup=True)
    assert [int(x) for x in dev[:, 0, 0, 0]] == [1, 2, 2, 2]   # image 1's two equal crops went up once
    assert len(fakes.taken) == 2 and len(fakes.events) == 1    # the chunk's buffer was released, the second one uploaded
    fakes.all_back_once()


@pytest.mark.parametrize("fail", ["allocation", "concatenate"])
def test_dedup_upload_that_raises_gives_both_buffers_back(fakes, monkeypatch, fail):
    st = stager(fakes)
    batch = st.stage([image(1), image(2, crops=3)], 8)
    batch.wait()
    if fail == "allocation":  # the one buffer is the chunk's: the unique crops need a new one
        fakes.fail_alloc = True
        with pytest.raises(MemoryError):
            consume(batch, st.ring, dedup=True)
        assert len(fakes.taken) == 1
    else:
        def concatenate(*args, **kwargs):
            raise ValueError("concatenate failed")

        with monkeypatch.context() as m:
            m.setattr(np, "concatenate", concatenate)
            with pytest.raises(ValueError, match="concatenate failed"):
                consume(batch, st.ring, dedup=True)
        assert len(fakes.taken) == 2
    assert not fakes.events
    fakes.all_back_once()


def test_stage_that_cannot_get_a_buffer_gives_back_what_it_took(fakes):
    st = stager(fakes)
    images = [image(i + 1) for i in range(4)]
    consume(st.stage(images[:2], 4), st.ring)   # one slot exists; the second chunk of the next batch needs another
    fakes.fail_alloc = True
    with pytest.raises(MemoryError):
        st.stage(images, 4)
    fakes.all_back_once()


# ------------------------------------------------------------------ batches staged ahead
def test_prefetch_table(fakes):
    st = stager(fakes)
    a, b, c = ([image(10 * k + i + 1) for i in range(3)] for k in range(3))
    st.prefetch(a, 4)
    st.prefetch(list(a), 4)                      # the same image objects: one entry
    assert len(st.prefetched) == 1 and len(fakes.taken) == 2
    st.prefetch(b, 4)
    st.prefetch(c, 4)                            # a third batch: the oldest (a) is drained, its slots are free again
    st.wait_prefetched()
    assert list(st.prefetched) == [tuple(id(im) for im in x) for x in (b, c)]
    assert sum(s.busy for s in st.ring.slots) == 4 and len(fakes.returned) == 2
    # take() of the prefetched objects: the entry leaves the table and nothing new is staged
    taken = len(fakes.taken)
    batch = st.take(b, 4)
    assert len(fakes.taken) == taken and list(st.prefetched) == [tuple(id(im) for im in c)]
    assert [int(d[0, 0, 0, 0]) for d in consume(batch, st.ring)] == [11, 13]
    # take() of copies: staged anew, the entry stays
    batch = st.take([im.copy() for im in c], 4)
    assert len(fakes.taken) == taken + 2 and len(st.prefetched) == 1
    assert [int(d[0, 0, 0, 0]) for d in consume(batch, st.ring)] == [21, 23]
    st.discard()
    assert not st.prefetched
    fakes.all_back_once()


