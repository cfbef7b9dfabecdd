"""The guarded allocator of tests/_guarded.py detects what it is there to detect (CPU: the device predicate accepts CPU tensors,
and every planted write lands inside the big buffer, so nothing faults)."""
import pytest
import torch

from _guarded import ALIGN, FINITE_FILL, GUARD, NAN_FILL, PATTERNS, guarded, hygiene, place

CPU = torch.device("cpu")
accept_cpu = lambda dev: dev.type == "cpu"  # noqa: E731


def _x():
    return torch.arange(1, 13, dtype=torch.float32).reshape(3, 4) / 8


def clean(put):
    x = put(_x())
    out = torch.empty_like(x)
    out.copy_(x * 2)
    return out


def writes_one_past(put):
    x = put(_x())
    out = torch.empty(x.shape, dtype=torch.float32)
    out.copy_(x * 2)
    if out._base is not None:  # a guarded allocation: the stray write lands in the big buffer (torch refuses it on a plain tensor)
        torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)
    return out


def writes_one_before(put):
    x = put(_x())
    out = x.new_empty(x.shape)
    out.copy_(x * 2)
    if out._base is not None:
        torch.as_strided(out, (1,), (1,), out.storage_offset() - 1).fill_(1.0)
    return out


def reads_unwritten_scratch(put):
    x = put(_x())
    out, scratch = torch.empty_like(x), torch.empty_like(x)
    if scratch._base is None:
        scratch.zero_()  # the plain run stands for the test process whose allocator happens to hand back zeros
    out.copy_(x * 2)
    return out + scratch


def reads_one_past_input(put):
    x = put(_x())
    row = torch.as_strided(x, (x.numel() + 1,), (1,), x.storage_offset())
    return row.sum().reshape(1)


def test_clean_function_passes():
    out = hygiene(clean, CPU, accept=accept_cpu)
    assert torch.equal(out, _x() * 2)


@pytest.mark.parametrize("fn,message", [
    (writes_one_past, "back guard of the empty allocated at"),
    (writes_one_before, "front guard of the empty allocated at"),
])
def test_write_outside_the_output_trips_the_guard_check(fn, message):
    with pytest.raises(AssertionError, match=message) as e:
        hygiene(fn, CPU, accept=accept_cpu)
    assert "test_guarded_cpu.py:" in str(e.value)  # the allocation site is named


def test_unwritten_scratch_trips_finiteness_then_equality():
    with pytest.raises(AssertionError, match="fill 0xFF: result 0 .* is not finite"):
        hygiene(reads_unwritten_scratch, CPU, accept=accept_cpu)
    with pytest.raises(AssertionError, match="fill 0x47: result 0 .* differs from the plain run"):
        hygiene(reads_unwritten_scratch, CPU, accept=accept_cpu, patterns=(FINITE_FILL,))


def test_read_past_a_placed_input_trips_finiteness_then_equality():
    with pytest.raises(AssertionError, match="fill 0xFF: result 0 .* is not finite"):
        hygiene(reads_one_past_input, CPU, accept=accept_cpu)
    with pytest.raises(AssertionError, match="fill 0x47: result 0 .* differs from the plain run"):
        hygiene(reads_one_past_input, CPU, accept=accept_cpu, patterns=(FINITE_FILL,))


def test_layout_alignment_and_fill():
    with guarded(NAN_FILL, accept=accept_cpu) as g:
        t = torch.empty((3, 5), dtype=torch.float32)
        u = torch.empty(7, dtype=torch.uint8)
        i = torch.empty(4, dtype=torch.int64)
        h = torch.empty_like(t, dtype=torch.float16)
        s = place(_x(), CPU, skew=4)
        for v in (t, u, i, h):
            assert v.data_ptr() % ALIGN == 0 and v.is_contiguous()
        assert s.data_ptr() % ALIGN == 4 and torch.equal(s, _x())
        assert torch.isnan(t).all() and torch.isnan(h).all() and (u == 0xFF).all()
        assert g.is_poisoned(t) and not g.is_poisoned(s)
        assert [b.big.numel() for b in g.buffers] == [2 * GUARD + 2 * ALIGN] * 5
        assert all(GUARD <= b.lo < GUARD + ALIGN + 4 and b.big.numel() - b.hi >= GUARD for b in g.buffers)
        g.check()
        i.fill_(3)  # an integer payload is the test's to use; its guards still hold
        g.check()
    with guarded(FINITE_FILL, accept=accept_cpu) as g:
        t, h = torch.empty(2, 2), torch.empty(2, dtype=torch.float16)
        assert 5.0e4 < float(t[0, 0]) < 5.2e4 and 7.0 < float(h[0]) < 7.5
    assert PATTERNS == (0xFF, 0x47)


def test_integer_payloads_and_index_scratch_are_not_poisoned():
    def train_queries():  # stands for the allocation site ops.train_queries (matched by file name, function and dtype)
        return torch.empty(64, dtype=torch.uint8), torch.empty((2, 5), dtype=torch.float32)

    with guarded(NAN_FILL, accept=accept_cpu, guards_only=(("test_guarded_cpu.py", "train_queries", torch.uint8),)) as g:
        probe = torch.empty(64, dtype=torch.uint8)
        ws, hr_coord = train_queries()
        assert g.is_poisoned(probe)
        bw, bf = g.buffers[-2], g.buffers[-1]
        assert not bw.poisoned and (bw.big[:bw.lo] == 0xFF).all() and (bw.big[bw.hi:] == 0xFF).all()
        assert bf.poisoned and g.is_poisoned(hr_coord) and torch.isnan(hr_coord).all()  # the function's float outputs are poisoned
        ws.fill_(0)
        g.check()
    from _guarded import _GUARDS_ONLY_SITES
    assert _GUARDS_ONLY_SITES == (("ops.py", "train_queries", torch.uint8),)
    with guarded(NAN_FILL, accept=accept_cpu) as g:
        base = torch.zeros(64, dtype=torch.int32)
        idx = torch.empty_like(base)
        b = g.buffers[-1]
        assert idx.dtype == torch.int32 and (b.big[:b.lo] == 0xFF).all() and (b.big[b.hi:] == 0xFF).all()
        torch.as_strided(idx, (1,), (1,), idx.storage_offset() + idx.numel()).fill_(1)
        with pytest.raises(AssertionError, match="back guard"):
            g.check()


def test_other_allocations_pass_through_and_patching_is_undone():
    orig = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with guarded(NAN_FILL) as g:  # the default predicate: CUDA / HIP devices only
        assert torch.empty(4).device.type == "cpu" and torch.empty(4, device="meta").device.type == "meta"
        assert not g.buffers
    with guarded(NAN_FILL, accept=accept_cpu) as g:
        cl = torch.empty((1, 3, 4, 5), memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last)
        nc = torch.empty_like(torch.zeros(4, 6).t())
        assert nc.stride() == (1, 6)
        torch.empty(3, out=torch.zeros(3))
        assert not g.buffers
        torch.empty(2, 3), torch.empty((2, 3)), torch.zeros(2).new_empty((5,)), torch.empty(size=(2,))
        assert len(g.buffers) == 4
        import numpy as np
        a = torch.empty((np.int64(2), torch.tensor(3)))  # sizes that are not Python ints are guarded too
        b = torch.zeros(2).new_empty(np.int32(4))
        assert len(g.buffers) == 6 and a.shape == (2, 3) and b.shape == (4,) and g.is_poisoned(a) and g.is_poisoned(b)
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig
    with pytest.raises(ZeroDivisionError):
        with guarded(NAN_FILL, accept=accept_cpu):
            1 / 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig


def test_every_library_symbol_has_a_hygiene_row_or_an_exemption():
    """EXEMPT ∪ {the table rows' symbols} == SIGNATURES, and nothing that takes a stream and a tensor pointer is exempt: a symbol
    added later fails here until tests/test_memory_hygiene_gpu.py gives it a row."""
    import ctypes as C

    from anystereo import _lib as L

    import test_memory_hygiene_gpu as H
    assert set(H.EXEMPT) | H.ROW_SYMBOLS == set(L.SIGNATURES), (sorted(set(L.SIGNATURES) - set(H.EXEMPT) - H.ROW_SYMBOLS),
                                                                sorted((set(H.EXEMPT) | H.ROW_SYMBOLS) - set(L.SIGNATURES)))
    assert not set(H.EXEMPT) & H.ROW_SYMBOLS
    assert all(isinstance(why, str) and why.strip() for why in H.EXEMPT.values())
    pointers = (C.c_void_p, L._pp, C.POINTER(L.ConvDesc))
    for name in H.EXEMPT:
        _, args = L.SIGNATURES[name]
        launches = len(args) >= 2 and args[-1] is C.c_void_p and any(a in pointers for a in args[:-1])
        assert not launches, f"{name} takes a stream and a tensor pointer: it needs a row, not an exemption"
    assert len({r.name for r in H.ROWS}) == len(H.ROWS)
    for r in H.ROWS:  # a tolerance row cites the parity test it takes the tolerance from
        for t in ([r.tol] if isinstance(r.tol, tuple) else list((r.tol or {}).values())):
            assert len(t) == 3 and "::test_" in t[2], r.name


def test_nothing_written_needs_something_to_inspect():
    with guarded(NAN_FILL, accept=accept_cpu) as g:
        with pytest.raises(AssertionError, match="no poisoned allocation to inspect"):
            g.nothing_written()
        torch.empty(3, dtype=torch.int32)  # guards only: still nothing to inspect
        with pytest.raises(AssertionError, match="no poisoned allocation to inspect"):
            g.nothing_written()
        t = torch.empty(3)
        assert g.nothing_written() and g.nothing_written(since=1)
        with pytest.raises(AssertionError, match="no poisoned allocation to inspect"):
            g.nothing_written(since=2)
        t[1] = 0.0
        assert not g.nothing_written()


def test_buffers_go_back_zero_filled():
    with guarded(NAN_FILL, accept=accept_cpu) as g:
        t = torch.empty(5)
        big = g.buffers[0].big
        assert torch.isnan(t).all()
    assert not g.buffers and (big == 0).all() and (t == 0).all()
