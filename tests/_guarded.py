"""A guarded, poisoned allocator for tests: what a kernel does to memory that is not part of its result.

Every output and scratch buffer of the operator layer comes from `torch.empty`.  In a test process the caching allocator mostly
hands back zeros or an earlier correct result, so a kernel that reads a buffer nobody wrote, or that writes a row past its output,
goes unnoticed.  Inside `with guarded(pattern) as g:` the three allocating calls (`torch.empty`, `torch.empty_like`,
`torch.Tensor.new_empty`) return, for a contiguous allocation on the device under test, an interior view of a larger uint8 buffer:

    [ 64 KiB guard | payload, rounded up to 512 B | 64 KiB guard ]

(the payload on a 512-B boundary like any torch allocation; `skew` / `skew_sites` move it off that boundary on purpose), all of
it filled with one byte value.  `g.check()` asserts that every guard byte still holds that value (a write outside the
tensor), a NaN (0xFF) or finite garbage (0x47) in the result shows a read of unwritten memory, and `place` gives a test's inputs
the same neighbours, so that a read before or after an input shows as well.  The context keeps every buffer alive: the allocator
cannot recycle one into a later allocation and hide a bug.

Integer tensors (int32 / int64) get guards but keep the payload as allocated: an unwritten index that is poisoned would turn a
silent bug into a wild address.  The same holds for the allocations named in `guards_only` by (file, function, dtype): the uint8
sparse-mode scratch of ops.train_queries, which holds pixel lists and counters — and nothing else that function allocates.

This is a helper module (like tests/_conv_cases.py), not a plugin: nothing is patched outside a `with` block.
"""
from __future__ import annotations

import contextlib
import operator
import os
import sys

import torch

GUARD = 64 * 1024   # bytes before and after every payload: more than any whole tensor plane at the suite's hygiene shapes
ALIGN = 512         # a torch allocation's alignment, kept by the payload
NAN_FILL = 0xFF     # NaN as fp16, fp32 and fp64
FINITE_FILL = 0x47  # ~5.1e4 as fp32, ~7.3 as fp16: finite garbage that fmaxf / ReLU / a comparison does not swallow as they do NaN
PATTERNS = (NAN_FILL, FINITE_FILL)

_POISONED = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8)
# (file name, function, dtype) of the allocations that get guards only: the uint8 scratch of the sparse modes of ops.train_queries,
# which holds pixel lists and counters (its float outputs, allocated in the same function, are poisoned like any other)
_GUARDS_ONLY_SITES = (("ops.py", "train_queries", torch.uint8),)
_THIS = os.path.abspath(__file__)
_ACTIVE = []  # innermost guarded context last

_orig_empty, _orig_empty_like, _orig_new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _caller():
    """(file, line, function) of the first frame outside this module."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _THIS:
        f = f.f_back
    if f is None:
        return "?", 0, "?"
    return f.f_code.co_filename, f.f_lineno, f.f_code.co_name


class _Buffer:
    __slots__ = ("big", "lo", "hi", "site", "kind", "poisoned")

    def __init__(self, big, lo, hi, site, kind, poisoned):
        self.big, self.lo, self.hi, self.site, self.kind, self.poisoned = big, lo, hi, site, kind, poisoned


class guarded:
    """with guarded(0xFF) as g: out = op(g.place(x, dev)); g.check()

    `accept(device) -> bool` says which device is under test (default: any CUDA / HIP device)."""

    def __init__(self, pattern: int, accept=None, guards_only=_GUARDS_ONLY_SITES, skew_sites=None):
        assert 0 <= int(pattern) <= 255
        self.pattern = int(pattern)
        self.accept = accept if accept is not None else (lambda dev: dev.type == "cuda")
        self.guards_only = tuple(guards_only)
        # (file name, function, dtype) -> bytes: allocations of that site start that far past their 512-B boundary (an output or
        # scratch buffer the op allocates itself, off the alignment a kernel chooses its path by)
        self.skew_sites = dict(skew_sites or {})
        self.buffers = []

    # ---- the context ----------------------------------------------------------------------------------------------------------
    def __enter__(self):
        if not _ACTIVE:
            torch.empty, torch.empty_like, torch.Tensor.new_empty = _patched_empty, _patched_empty_like, _patched_new_empty
        _ACTIVE.append(self)
        return self

    def __exit__(self, *exc):
        _ACTIVE.remove(self)
        if not _ACTIVE:
            torch.empty, torch.empty_like, torch.Tensor.new_empty = _orig_empty, _orig_empty_like, _orig_new_empty
        # leave the caching allocator as the rest of the suite has always found it: the blocks go back zero-filled, not holding the
        # poison (so: compare a guarded run's results INSIDE the context, or clone them there)
        for b in self.buffers:
            b.big.zero_()
        self.buffers = []
        return False

    # ---- allocation -----------------------------------------------------------------------------------------------------------
    def _carve(self, shape, dtype, device, site, kind, poison: bool, skew: int = 0):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        esize = torch.empty((), dtype=dtype, device="meta").element_size()
        assert skew % esize == 0, f"skew {skew} is no multiple of the element size {esize}"
        nbytes = numel * esize
        total = GUARD + _round_up(skew + nbytes, ALIGN) + GUARD
        big = _orig_empty(total + ALIGN, dtype=torch.uint8, device=device)
        lo = GUARD + (-big.data_ptr()) % ALIGN + skew  # a device allocation is 512-B aligned already; a host one need not be
        hi = lo + nbytes
        if poison:
            big.fill_(self.pattern)
        else:  # guards only: the payload stays as the allocator gave it
            big[:lo].fill_(self.pattern)
            big[hi:].fill_(self.pattern)
        self.buffers.append(_Buffer(big, lo, hi, site, kind, poison))
        flat = big[lo:hi]
        view = flat.view(torch.uint8 if dtype == torch.bool else dtype)
        if dtype == torch.bool:
            view = view.view(torch.bool)
        return view.view(shape)

    def _alloc(self, shape, dtype, device, requires_grad=False):
        fname, line, func = _caller()
        site = f"{os.path.relpath(fname) if os.path.isabs(fname) else fname}:{line}"
        poison = dtype in _POISONED and (os.path.basename(fname), func, dtype) not in self.guards_only
        t = self._carve(shape, dtype, device, site, "empty", poison, self.skew_sites.get((os.path.basename(fname), func, dtype), 0))
        if requires_grad:
            t.requires_grad_(True)
        return t

    def place(self, t: torch.Tensor, dev, skew: int = 0) -> torch.Tensor:
        """A copy of the host tensor `t` on `dev` with poisoned neighbours; `skew` bytes move the payload off its 512-B boundary."""
        fname, line, _ = _caller()
        site = f"{os.path.relpath(fname) if os.path.isabs(fname) else fname}:{line}"
        src = t.detach().contiguous()
        view = self._carve(src.shape, src.dtype, torch.device(dev), site, "placed input", True, skew)
        view.copy_(src)
        return view

    # ---- the check ------------------------------------------------------------------------------------------------------------
    def check(self) -> None:
        """Every guard byte still holds the fill value: reductions on the device, one synchronisation at the end."""
        if not self.buffers:
            return
        flags = []
        for b in self.buffers:
            flags.append((b.big[:b.lo] != self.pattern).any())
            flags.append((b.big[b.hi:] != self.pattern).any())
        by_dev = {}
        for i, f in enumerate(flags):
            by_dev.setdefault(f.device, []).append((i, f))
        hit = [False] * len(flags)
        for dev, fs in by_dev.items():
            got = torch.stack([f for _, f in fs]).cpu().tolist()
            for (i, _), v in zip(fs, got):
                hit[i] = bool(v)
        bad = []
        for k, b in enumerate(self.buffers):
            for side, h in (("front", hit[2 * k]), ("back", hit[2 * k + 1])):
                if h:
                    bad.append(f"{side} guard of the {b.kind} allocated at {b.site} ({b.hi - b.lo} bytes) was overwritten")
        assert not bad, f"guard bytes changed under fill 0x{self.pattern:02X}: " + "; ".join(bad)

    def nothing_written(self, since: int = 0) -> bool:
        """Every poisoned allocation made inside the context (from buffer number `since` on) still holds the fill value in every
        byte: nothing was launched on it.  It is an error to ask when there is no such allocation: the answer would say nothing."""
        flags = [(b.big[b.lo:b.hi] != self.pattern).any() for b in self.buffers[since:] if b.kind == "empty" and b.poisoned and b.hi > b.lo]
        assert flags, "nothing_written: no poisoned allocation to inspect"
        return not bool(torch.stack(flags).any().item())

    def is_poisoned(self, t: torch.Tensor) -> bool:
        """Every byte of `t` (a guarded, poisoned allocation) still holds the fill value: nothing wrote it."""
        return bool((t.contiguous().view(-1).view(torch.uint8) == self.pattern).all().item())


# ---- the patched allocating calls ---------------------------------------------------------------------------------------------

def _default_device() -> torch.device:
    get = getattr(torch, "get_default_device", None)
    return get() if get is not None else torch.device("cpu")


def _resolve(device) -> torch.device:
    dev = _default_device() if device is None else torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _plain_kwargs(kw, like_contiguous=True) -> bool:
    """True when the keyword arguments ask for an ordinary strided, pageable, contiguous allocation."""
    if kw.get("out") is not None or kw.get("names") is not None or kw.get("pin_memory"):
        return False
    if kw.get("layout") not in (None, torch.strided):
        return False
    mf = kw.get("memory_format")
    if mf is None or mf == torch.contiguous_format:
        return True
    return mf == torch.preserve_format and like_contiguous


def _size_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0])
    return tuple(args)


def _ints(size):
    """The size as Python ints: numpy integers, 0-d integer tensors and symbolic ints are coerced through __index__, so that such a
    site is guarded like any other.  None only for what torch.empty itself rejects as a size (it then raises the error)."""
    try:
        return tuple(operator.index(s) for s in size)
    except TypeError:
        return None


def _patched_empty(*args, **kw):
    g = _ACTIVE[-1] if _ACTIVE else None
    if g is not None and _plain_kwargs(kw, like_contiguous=False):
        size = _ints(kw["size"] if "size" in kw else _size_of(args))
        if size is not None:
            dev = _resolve(kw.get("device"))
            if g.accept(dev):
                return g._alloc(size, kw.get("dtype") or torch.get_default_dtype(), dev, bool(kw.get("requires_grad")))
    return _orig_empty(*args, **kw)


def _patched_empty_like(t, **kw):
    g = _ACTIVE[-1] if _ACTIVE else None
    if (g is not None and isinstance(t, torch.Tensor) and t.layout == torch.strided and t.is_contiguous()
            and _plain_kwargs(kw, like_contiguous=True)):
        dev = _resolve(kw["device"]) if kw.get("device") is not None else t.device
        if g.accept(dev):
            return g._alloc(t.shape, kw.get("dtype") or t.dtype, dev, bool(kw.get("requires_grad")))
    return _orig_empty_like(t, **kw)


def _patched_new_empty(self, *args, **kw):
    g = _ACTIVE[-1] if _ACTIVE else None
    if g is not None and self.layout == torch.strided and _plain_kwargs(kw, like_contiguous=False):
        size = _ints(kw["size"] if "size" in kw else _size_of(args))
        if size is not None:
            dev = _resolve(kw["device"]) if kw.get("device") is not None else self.device
            if g.accept(dev):
                return g._alloc(size, kw.get("dtype") or self.dtype, dev, bool(kw.get("requires_grad")))
    return _orig_new_empty(self, *args, **kw)


# ---- placing inputs -----------------------------------------------------------------------------------------------------------

def place(t: torch.Tensor, dev, skew: int = 0) -> torch.Tensor:
    """Copy the host tensor `t` into the interior of a guarded buffer on `dev` and return the view.  Inside a guarded context the
    neighbours hold its fill value and its check covers them; outside one they hold zeros (the plain run of a comparison)."""
    if _ACTIVE:
        return _ACTIVE[-1].place(t, dev, skew)
    return _ZERO.place(t, dev, skew)


class _ZeroFill(guarded):
    """place() outside a context: the same layout with a zero fill; nothing is registered, the view keeps its buffer alive."""

    def place(self, t, dev, skew: int = 0):
        view = super().place(t, dev, skew)
        self.buffers.clear()
        return view


_ZERO = _ZeroFill(0)


# ---- counting the calls made under a guard ------------------------------------------------------------------------------------

@contextlib.contextmanager
def counted(L, calls: dict):
    """For the duration of the block every function of `L.SIGNATURES` on the loaded library `L.load()` (a binding module:
    anystereo._lib, _scenes_lib, ...) counts into `calls[name]` the calls made while a guarded context is active; the functions
    themselves are put back on exit.  A module's "every launching symbol was called under a guard" test reads `calls`."""
    lib = L.load()
    orig = {n: getattr(lib, n) for n in L.SIGNATURES}

    def wrap(name, fn):
        def call(*a):
            if _ACTIVE:
                calls[name] = calls.get(name, 0) + 1
            return fn(*a)
        return call
    for n, fn in orig.items():
        setattr(lib, n, wrap(n, fn))
    try:
        yield
    finally:
        for n, fn in orig.items():
            setattr(lib, n, fn)


# ---- the three-run comparison -------------------------------------------------------------------------------------------------

def flatten(out):
    """The tensors of an op's result: a tensor, None, an object with a `.t` tensor (a blocked split-fp16 buffer), or a nest of those."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if hasattr(out, "t") and isinstance(out.t, torch.Tensor):
        return [out.t]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in flatten(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in flatten(o)]
    raise TypeError(f"hygiene: cannot compare a result of type {type(out).__name__}")


def _finite(t: torch.Tensor) -> bool:
    return True if not t.is_floating_point() else bool(torch.isfinite(t).all().item())


def hygiene(fn, dev, accept=None, compare=None, patterns=PATTERNS):
    """Run `fn(put)` three times — plain (inputs placed with a zero fill, no patching), under guarded(0xFF) and under
    guarded(0x47) — where `put(t, skew=0)` places a host tensor on `dev`.  Asserts that all guards are intact in both guarded runs
    (those around the inputs included), that every returned tensor is finite, and that every returned tensor is the same in all
    three runs: bit-equal, or `compare(got, want, what)` for an entry whose kernel accumulates with float atomics.
    Returns the plain run's result."""
    put = lambda t, skew=0: place(t, dev, skew)  # noqa: E731
    plain = fn(put)
    want = [t.detach().clone() for t in flatten(plain)]
    for i, t in enumerate(want):
        assert _finite(t), f"plain run: result {i} is not finite"
    for pattern in patterns:
        with guarded(pattern, accept=accept) as g:
            got = flatten(fn(put))
            g.check()
            assert len(got) == len(want), f"fill 0x{pattern:02X}: {len(got)} results, the plain run gave {len(want)}"
            for i, (a, b) in enumerate(zip(got, want)):
                what = f"fill 0x{pattern:02X}: result {i} {tuple(a.shape)} {a.dtype}"
                assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: the plain run gave {tuple(b.shape)} {b.dtype}"
                assert _finite(a), f"{what} is not finite: the op read memory nobody wrote"
                if compare is None:
                    assert torch.equal(a, b), (f"{what} differs from the plain run in {int((a != b).sum())} of {a.numel()} elements: "
                                               "the op read memory nobody wrote")
                else:
                    compare(a, b, what)
    return plain
