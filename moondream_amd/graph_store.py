"""What ``compile()`` switches on, under one owner: the captured decode graphs and the device buffers whose addresses they
bake in.  A captured chunk replays its launches with the addresses they had at capture, so
  * a buffer a chunk addresses is made by this store only: ``fixed`` (one per key, never replaced) or ``grow`` (one per
    name, replaced when a caller asks for more);
  * ``grow`` replacing a buffer drops every graph (``invalidate``), as does whoever reallocates the one thing kept
    elsewhere, the KV slab;
  * ``invalidate`` drops graphs only: buffers stay alive (work queued on another stream may still address them).
Host only: no kernels, no model, no torch; the device synchronise and the capture are handed in (tests without a GPU).
"""
from __future__ import annotations

from types import MappingProxyType
from typing import Any, Callable, Dict, Hashable, Iterator, Mapping, Optional


class _GraphKeys:
    """The keys of the stored graphs, read-only but for ``clear`` (== ``invalidate``)."""

    __slots__ = ("_store",)

    def __init__(self, store: "GraphStore"):
        self._store = store

    def __len__(self) -> int:
        return len(self._store._graphs)

    def __iter__(self) -> Iterator:
        return iter(self._store._graphs)

    def __contains__(self, key) -> bool:
        return key in self._store._graphs

    def clear(self) -> None:
        self._store.invalidate()


class GraphStore:
    """``synchronize()`` waits for the device; ``capture(body)`` records ``body``'s launches without executing them and
    returns an object with ``replay()``."""

    def __init__(self, synchronize: Callable[[], None], capture: Callable[[Callable[[], None]], Any]):
        self._synchronize, self._capture = synchronize, capture
        self._graphs: Dict[Hashable, Any] = {}
        self._grown: Dict[Hashable, Any] = {}
        self._fixed: Dict[str, Dict[Hashable, Any]] = {}

    @property
    def graphs(self) -> _GraphKeys:
        """(Made per read: a view kept here would be a reference cycle, and the graphs and buffers of a dropped model
        would wait for the collector instead of going with it.)"""
        return _GraphKeys(self)

    def replay_or_capture(self, key, body: Callable[[], None], may_capture: Optional[Callable[[], bool]] = None) -> bool:
        """Replay the graph stored under ``key``; a key not seen before runs ``body`` eagerly, then captures it and stores
        the graph.  An eager warm-up on scratch state is not possible (KV side effects), so the first chunk of a new shape
        IS the eager run and the graph is captured after a device synchronise; the capture does not execute, there is
        nothing to undo.  ``may_capture`` (asked on a miss only): False runs eagerly without storing.  Returns True when
        it captured."""
        graph = self._graphs.get(key)
        if graph is not None:
            graph.replay()
            return False
        body()
        if may_capture is not None and not may_capture():
            return False
        self._synchronize()
        self._graphs[key] = self._capture(body)
        return True

    def count(self, tag, stream) -> int:
        """Stored graphs whose key starts (``tag``, ``stream``)."""
        return sum(1 for k in self._graphs if isinstance(k, tuple) and k[:2] == (tag, stream))

    def invalidate(self) -> None:
        """Drop every graph: something its launches baked in is about to change."""
        self._graphs.clear()

    def grow(self, name: Hashable, size: int, make: Callable[[], Any]):
        """The buffer of ``name`` when ``len`` of it is at least ``size``; otherwise ``make()`` (the caller's allocation,
        with its own head room) takes its place and every graph is dropped."""
        buf = self._grown.get(name)
        if buf is None or len(buf) < size:
            buf = self._grown[name] = make()
            self.invalidate()
        return buf

    def fixed(self, namespace: str, key: Hashable, make: Callable[[], Any]):
        """The buffers of ``key`` in ``namespace``: made on first use, the same object from then on."""
        bufs = self._fixed.setdefault(namespace, {})
        if key not in bufs:
            bufs[key] = make()
        return bufs[key]

    def fixed_view(self, namespace: str) -> Mapping:
        """Read-only: key -> buffers of ``namespace``."""
        return MappingProxyType(self._fixed.setdefault(namespace, {}))

    def forget_fixed(self, namespace: str) -> None:
        """Tests only: start ``namespace`` empty.  The graphs go too: they address what is forgotten."""
        self.invalidate()
        self._fixed.setdefault(namespace, {}).clear()
