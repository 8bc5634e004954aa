"""The graph store (moondream_amd/graph_store.py) without a GPU: the synchronise counts its calls, "capturing" records
the body and runs nothing, and buffers are objects with a size and an address."""
import itertools

import pytest

from moondream_amd.graph_store import GraphStore


class Buf:
    _next = itertools.count(0x1000, 0x1000)

    def __init__(self, size):
        self.size, self.addr = size, next(Buf._next)

    def __len__(self):
        return self.size


class Harness:
    """A store over fakes, and everything they saw, in order."""

    def __init__(self):
        self.events, self.made = [], []
        self.store = GraphStore(lambda: self.events.append("sync"), self.capture)

    def capture(self, body):
        self.events.append(("capture", body))
        return self  # the "graph"

    def replay(self):
        self.events.append("replay")

    def body(self, name="body"):
        return lambda: self.events.append(name)

    def alloc(self, size):
        def make():
            self.made.append(Buf(size))
            return self.made[-1]

        return make


@pytest.fixture
def h():
    return Harness()


def test_a_miss_runs_eagerly_once_then_synchronises_then_captures(h):
    body = h.body()
    assert h.store.replay_or_capture("k", body) is True
    assert h.events == ["body", "sync", ("capture", body)]
    assert "k" in h.store.graphs and len(h.store.graphs) == 1


def test_a_hit_replays_without_running_the_body_or_asking(h):
    h.store.replay_or_capture("k", h.body())
    del h.events[:]
    asked = []
    assert h.store.replay_or_capture("k", h.body(), may_capture=lambda: asked.append(1) or True) is False
    assert h.events == ["replay"] and asked == []


def test_a_refused_capture_runs_once_and_stores_nothing(h):
    asked = []
    assert h.store.replay_or_capture("k", h.body(), may_capture=lambda: asked.append(1) and False) is False
    assert h.events == ["body"] and asked == [1]
    assert "k" not in h.store.graphs and len(h.store.graphs) == 0
    assert h.store.replay_or_capture("k", h.body(), may_capture=lambda: True) is True  # still a miss, and now allowed


def test_grow_keeps_a_buffer_that_is_large_enough(h):
    a = h.store.grow("logits", 8, h.alloc(10))
    h.store.replay_or_capture("k", h.body())
    for size in (1, 8, 10):  # up to what was made, not what was asked for
        assert h.store.grow("logits", size, h.alloc(size)) is a
    assert len(h.made) == 1 and list(h.store.graphs) == ["k"]


def test_grow_replaces_a_buffer_that_is_too_small_and_drops_the_graphs(h):
    a = h.store.grow("variants", 2, h.alloc(2))
    other = h.store.grow(("arena", 2), 100, h.alloc(100))
    h.store.replay_or_capture("k1", h.body())
    h.store.replay_or_capture("k2", h.body())
    b = h.store.grow("variants", 3, h.alloc(3))
    assert b is not a and b.addr != a.addr and len(b) == 3 and len(h.made) == 3  # ``make`` ran once more, once
    assert len(h.store.graphs) == 0 and "k1" not in h.store.graphs
    assert h.store.grow("variants", 3, h.alloc(3)) is b
    assert h.store.grow(("arena", 2), 100, h.alloc(100)) is other  # another name's buffer stays
    assert len(h.made) == 3


def test_fixed_is_one_object_per_namespace_and_key_and_outlives_the_graphs(h):
    a = h.store.fixed("chunk", (0x11, 2, 4), h.alloc(8))
    assert h.store.fixed("chunk", (0x11, 2, 4), h.alloc(8)) is a and len(h.made) == 1
    b = h.store.fixed("chunk", (0x22, 2, 4), h.alloc(8))  # another stream only
    c = h.store.fixed("reason", (0x11, 2, 4), h.alloc(8))  # another namespace only
    assert len({a.addr, b.addr, c.addr}) == 3
    h.store.replay_or_capture("k", h.body())
    h.store.invalidate()
    h.store.grow("logits", 1, h.alloc(1))
    assert h.store.fixed("chunk", (0x11, 2, 4), h.alloc(8)) is a and h.store.fixed("chunk", (0x22, 2, 4), h.alloc(8)) is b
    assert set(h.store.fixed_view("chunk")) == {(0x11, 2, 4), (0x22, 2, 4)} and h.store.fixed_view("chunk")[0x22, 2, 4] is b
    with pytest.raises(TypeError):
        h.store.fixed_view("chunk")[0x33, 2, 4] = a
    h.store.forget_fixed("chunk")
    assert len(h.store.fixed_view("chunk")) == 0 and h.store.fixed("reason", (0x11, 2, 4), h.alloc(8)) is c


def test_count_and_the_continuous_engines_cap(h):
    cap, s0, s1 = 2, 0x11, 0x22
    run = lambda key: h.store.replay_or_capture(key, h.body(), lambda: h.store.count(key[0], key[1]) < cap)
    assert run(("continuous", s0, 1)) and run(("continuous", s0, 2))
    assert run(("decode", s0, 1)) and h.store.replay_or_capture("not a tuple", h.body())
    assert h.store.count("continuous", s0) == 2 and h.store.count("decode", s0) == 1 and h.store.count("continuous", s1) == 0
    del h.events[:]
    assert run(("continuous", s0, 3)) is False  # a third shape on the stream: eager, not stored
    assert h.events == ["body"] and ("continuous", s0, 3) not in h.store.graphs
    assert run(("continuous", s1, 3)) is True  # another stream has its own count
    assert run(("continuous", s0, 1)) is False and h.events[-1] == "replay"  # at the cap the stored ones still replay
    assert h.store.count("continuous", s0) == 2 and h.store.count("continuous", s1) == 1


def test_the_key_view_reads_the_graphs_and_clears_like_invalidate(h):
    view = h.store.graphs
    for k in ("a", ("decode", 1), ("decode", 2)):
        h.store.replay_or_capture(k, h.body())
    assert len(view) == 3 and list(view) == ["a", ("decode", 1), ("decode", 2)] and ("decode", 2) in view and "b" not in view
    assert not hasattr(view, "__setitem__") and not hasattr(view, "pop")
    buf = h.store.fixed("chunk", 1, h.alloc(1))
    view.clear()
    assert len(view) == 0 and list(view) == [] and h.store.count("decode", 1) == 0
    h.store.replay_or_capture("a", h.body())
    h.store.invalidate()
    assert len(view) == 0 and "a" not in view
    assert h.store.fixed("chunk", 1, h.alloc(1)) is buf  # neither drops a buffer


def test_a_dropped_store_frees_its_graphs_and_buffers_at_once():
    """By reference count, not by the cycle collector: a model that goes out of scope gives its device memory back then."""
    import gc
    import weakref

    class Graph:
        pass

    gc.disable()
    try:
        store = GraphStore(lambda: None, lambda body: Graph())
        alive = [weakref.ref(store.grow("logits", 1, lambda: Buf(1))), weakref.ref(store.fixed("chunk", 1, lambda: Buf(1)))]
        store.replay_or_capture("k", lambda: None)
        view = store.graphs
        alive.append(weakref.ref(store._graphs["k"]))
        assert len(view) == 1 and len(store.graphs) == 1
        del store, view
        assert [r() for r in alive] == [None, None, None]
    finally:
        gc.enable()


def test_the_module_is_host_only():
    import moondream_amd.graph_store as gs

    imports = [ln.split()[1] for ln in open(gs.__file__).read().splitlines() if ln.startswith(("import ", "from "))]
    assert imports == ["__future__", "types", "typing"]  # neither torch nor _lib nor the model
