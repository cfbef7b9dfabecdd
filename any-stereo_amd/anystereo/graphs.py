"""Captured passes: the one home of the inference hipGraph capture-and-replay cache (models/base.py: forward and encode).

A replay runs no Python: it reads the buffers that existed at capture time.  So a captured pass is selected by a key that names
everything it baked in (`GraphKey`), lives in an LRU (`GraphCache`: each entry holds a private memory pool with a whole pass) and
keeps alive what its nodes address but its pool does not own (`CapturedPass.refs`, and the `Stamps` object inside its key)."""
from __future__ import annotations

import os
from typing import NamedTuple


def tensors_fingerprint(tensors):
    """-> (count, sum of version counters, xor of position-salted addresses): changes with an in-place update, a replaced tensor,
    .to() / .half().  Not seen: writes through `.data` (they do not bump the version counter)."""
    ver = ptr = n = 0
    for t in tensors:
        ver += t._version
        ptr ^= (t.data_ptr() + 0x9E3779B97F4A7C15 * n) & 0xFFFFFFFFFFFFFFFF
        n += 1
    return (n, ver, ptr)


class GraphCache:
    """LRU over hashable keys (dict order = recency, least recently used first)."""

    def __init__(self):
        self._entries = {}

    def get(self, key):
        """The entry (now the most recently used one) or None."""
        ent = self._entries.pop(key, None)
        if ent is not None:
            self._entries[key] = ent
        return ent

    def put(self, key, entry, size):
        """Insert as most recently used; at most max(1, size) entries stay."""
        self._entries.pop(key, None)
        while len(self._entries) >= max(1, size):
            self._entries.pop(next(iter(self._entries)))
        self._entries[key] = entry

    def clear(self):
        self._entries.clear()

    def values(self):
        return self._entries.values()

    def __len__(self):
        return len(self._entries)

    def __iter__(self):
        return iter(self._entries)


class GraphKey(NamedTuple):
    """What a captured inference pass baked in.  `stamps` is the ops.Stamps object itself (hashed by identity), not its id(): the
    cached key keeps it alive, so no later Stamps can take its id while a graph that writes into its buffer exists."""
    kind: str  # "forward" | "encode"
    shapes: tuple
    at: object  # encode: the kept iterations; forward: None
    iters: int
    device: object
    precision: str
    fast16: bool
    weights: tuple
    stamps: object


class CapturedPass:
    """graph; static = the input clones its nodes read; out = what the captured function returned (tensors of the graph's pool);
    memsets = (replaced, left) of the memset rewrite, None where it did not run; refs = tensors the nodes address that the pool
    does not own."""
    __slots__ = ("graph", "static", "out", "memsets", "refs")

    def __init__(self, graph, static, out, memsets, refs):
        self.graph, self.static, self.out, self.memsets, self.refs = graph, static, out, memsets, refs

    def replay(self, *inputs):
        """-> `out`, overwritten by the next replay: the caller clones what it keeps."""
        for dst, src in zip(self.static, inputs):
            dst.copy_(src)
        self.graph.replay()
        return self.out


def capture_pass(fn, inputs, device, refs=()):
    """Capture fn(*clones of inputs) -> CapturedPass.  `refs`: tensors to keep alive with the graph, or a callable that returns them,
    evaluated after the capture.  If `fn` raises, the exception propagates and nothing is kept."""
    import torch

    from . import ops
    static = [t.detach().clone() for t in inputs]

    def load():  # fn may write its inputs (the forward clamps hr_coord in place): every call starts from the caller's values
        for dst, src in zip(static, inputs):
            dst.copy_(src)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: MIOpen solver search, weight packing, allocator
        for _ in range(2):
            load()
            fn(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize(device)
    keep = os.environ.get("ANYSTEREO_INFER_GRAPH_KEEP", "1") != "0"  # 0 (diagnostics): instantiate at capture end, no node rewrite
    g = torch.cuda.CUDAGraph(keep_graph=True) if keep else torch.cuda.CUDAGraph()
    load()
    with torch.cuda.graph(g):
        out = fn(*static)
    # memset nodes (a library zero-filling through hipMemsetAsync) are not reliably ordered inside long graphs on this ROCm stack
    # (csrc/graph.hip): rewritten as fill kernel nodes before instantiation.  This library issues none itself; the
    # count is kept for inspection.
    memsets = None
    if keep:
        memsets = ops.graph_replace_memsets(g)
        g.instantiate()
    return CapturedPass(g, static, out, memsets, tuple(refs() if callable(refs) else refs))
