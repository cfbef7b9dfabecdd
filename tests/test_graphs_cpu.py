"""CPU: the graph cache's selection rules (anystereo/graphs.py) without a GPU and without the native library — `GraphCache` (LRU),
`GraphKey` (the stamps object by identity, kept alive by the cached key), `tensors_fingerprint` against the formula written out here."""
import gc
import weakref

import pytest
import torch

from anystereo.graphs import GraphCache, GraphKey, tensors_fingerprint


def test_cache_hit_miss_recency_and_eviction():
    c = GraphCache()
    assert len(c) == 0 and c.get("a") is None and list(c) == []
    c.put("a", 1, 3)
    c.put("b", 2, 3)
    c.put("c", 3, 3)
    assert len(c) == 3 and list(c) == ["a", "b", "c"] and list(c.values()) == [1, 2, 3]
    assert c.get("a") == 1 and list(c) == ["b", "c", "a"]  # a hit is the most recent entry
    assert c.get("x") is None and list(c) == ["b", "c", "a"]  # a miss changes nothing
    c.put("d", 4, 3)  # "b" is the least recently used one
    assert list(c) == ["c", "a", "d"] and c.get("b") is None
    c.put("c", 33, 3)  # an existing key: replaced, most recent, nothing evicted
    assert list(c) == ["a", "d", "c"] and c.get("c") == 33
    c.clear()
    assert len(c) == 0 and list(c) == [] and c.get("a") is None


def test_cache_size_is_read_at_put_time():
    c = GraphCache()
    for i in range(4):
        c.put(i, i, 4)
    c.put(4, 4, 2)  # a smaller size now: down to 2 entries, the most recent ones
    assert list(c) == [3, 4]
    for size in (0, -5):  # below 1 counts as 1
        c.put("k", "v", size)
        assert list(c) == ["k"]
    c.put("l", "w", 3)
    assert list(c) == ["k", "l"]


class _Stamps:  # like ops.Stamps: no __eq__ / __hash__, so equal and hashed by identity
    pass


def _key(stamps, **over):
    f = dict(kind="forward", shapes=((1, 3, 64, 128), (1, 18432, 2), (1, 1)), at=None, iters=3, device=0, precision="split",
             fast16=False, weights=(10, 0, 1234), stamps=stamps)
    f.update(over)
    return GraphKey(**f)


def test_key_fields_and_stamps_identity():
    s1, s2 = _Stamps(), _Stamps()
    assert _key(s1) == _key(s1) and hash(_key(s1)) == hash(_key(s1))
    assert _key(s1) != _key(s2) and _key(s1) != _key(None)
    for over in (dict(kind="encode"), dict(at=(2, 3)), dict(iters=4), dict(device=1), dict(precision="fp32"), dict(fast16=True),
                 dict(weights=(10, 1, 1234)), dict(shapes=((1, 3, 64, 96),))):
        assert _key(s1, **over) != _key(s1), over
    k = _key(s1, kind="encode", at=(1, 3))
    assert (k.kind, k.at, k.iters, k.stamps) == ("encode", (1, 3), 3, s1) and k.stamps is s1
    c = GraphCache()
    c.put(_key(s1), "one", 2)
    c.put(_key(s2), "two", 2)
    assert len(c) == 2 and c.get(_key(s1)) == "one" and c.get(_key(s2)) == "two"


def test_cached_key_keeps_its_stamps_alive():
    c = GraphCache()
    s = _Stamps()
    ref = weakref.ref(s)
    c.put(_key(s), "entry", 1)
    del s
    gc.collect()
    assert ref() is not None and next(iter(c)).stamps is ref()  # no later object can take its id()
    c.put(_key(None), "other", 1)  # evicts it
    gc.collect()
    assert ref() is None


def _written_out(tensors):
    """What ContinuousStereoBase._weights_fingerprint computed before graphs.py existed."""
    ver = ptr = n = 0
    for t in tensors:
        ver += t._version
        ptr ^= t.data_ptr() + 0x9E3779B97F4A7C15 * n & 0xFFFFFFFFFFFFFFFF
        n += 1
    return (n, ver, ptr)


def test_tensors_fingerprint():
    ts = [torch.zeros(3, 5), torch.ones(7), torch.arange(4.0)]
    ts[1].add_(1.0)
    f0 = tensors_fingerprint(ts)
    assert f0 == _written_out(ts) == tensors_fingerprint(iter(ts)) and f0[0] == 3
    assert tensors_fingerprint([]) == (0, 0, 0)
    ts[0].mul_(2.0)  # an in-place update
    f1 = tensors_fingerprint(ts)
    assert f1 != f0 and f1 == _written_out(ts) and f1[1] == f0[1] + 1 and f1[2] == f0[2]
    keep = ts[2]
    ts[2] = keep.clone()  # a replaced tensor: another address
    f2 = tensors_fingerprint(ts)
    assert f2 != f1 and f2 == _written_out(ts)
    assert tensors_fingerprint([ts[1], ts[0], ts[2]]) != f2  # the address is salted with the position
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    assert tensors_fingerprint(list(m.parameters()) + list(m.buffers())) == _written_out(list(m.parameters()) + list(m.buffers()))


def test_model_fingerprint_is_the_shared_formula():
    from anystereo.models.base import ContinuousStereoBase

    class Tiny(ContinuousStereoBase):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 4, 3)
            self.bn = torch.nn.BatchNorm2d(4)

    m = Tiny()
    assert m._weights_fingerprint() == _written_out(list(m.parameters()) + list(m.buffers()))
    with torch.no_grad():
        m.conv.weight.add_(1.0)
    assert m._weights_fingerprint() == _written_out(list(m.parameters()) + list(m.buffers()))


def test_failed_construction_leaves_the_cache_unchanged():
    c = GraphCache()
    c.put("a", 1, 2)
    c.put("b", 2, 2)

    def lookup(key, build):  # the callers' pattern: get, on a miss build + put
        ent = c.get(key)
        if ent is None:
            ent = build()
            c.put(key, ent, 2)
        return ent

    def broken():
        raise RuntimeError("capture failed")

    with pytest.raises(RuntimeError, match="capture failed"):
        lookup("c", broken)
    assert list(c) == ["a", "b"] and list(c.values()) == [1, 2]
    assert lookup("c", lambda: 3) == 3 and list(c) == ["b", "c"]
