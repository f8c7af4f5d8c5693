"""A guarded stand-in for ``torch`` in the wrapper modules: every tensor a wrapper allocates sits between two guard bands.

The wrappers (uforecon_amd/ops.py, autograd.py, frustum.py, featurenet.py, optim.py) hand the library outputs and workspaces of
exactly the documented size.  torch's caching allocator rounds every request up to 512 bytes and packs small ones into shared
blocks, so a kernel that stores a few bytes past its output lands in slack or in a neighbour, and nothing fails.  A test
swaps a module's ``torch`` for a ``GuardedTorch``:

    g = GuardedTorch()
    monkeypatch.setattr(ops, "torch", g)
    out = ops.some_wrapper(g.place(x))
    g.check()

``GuardedTorch`` forwards every attribute to the real torch and replaces the allocating functions the wrappers use (``empty``,
``zeros``, ``ones``, ``full`` and their ``_like`` forms).  A request of ``nbytes`` (element count x element size, not rounded)
becomes one uint8 buffer of ``GUARD + nbytes + GUARD`` bytes from the real torch; both guards are filled with 0xFF -- NaN as
fp16 / bf16 / fp32 / fp64, -1 as any integer -- and the inner bytes come back viewed as the requested dtype and shape.  GUARD is
a multiple of 512, so the tensor has the alignment class of a fresh torch allocation (the 16-byte paths of the kernels are
the ones that run).  The inner bytes of a floating ``empty`` are 0xFF as well: a result that depends on memory the kernel
never wrote shows up as NaN.  Integer, uint8 and bool ``empty`` tensors are zero-filled: a stale integer used as an index must
not become a wild address.  ``zeros`` / ``ones`` / ``full`` hold what was asked.

``check()`` synchronises and asserts that every guard byte of every buffer still holds the pattern, naming the allocation
(call site, shape, dtype, which guard, first and last damaged byte relative to the inner region) otherwise.  ``place(t)``
copies a test input into a guarded buffer: a kernel that reads past an input reads NaN or -1.

Tensor methods (``x.new_zeros``, ``x.clone()``, ``x.contiguous()``, ``torch.sort`` ...) are not intercepted: what they return is
unguarded.  The patch lives inside the test that installs it; nothing here touches the allocator or the process.
"""
from __future__ import annotations

import os
import sys

import torch as _torch

GUARD = 4096            # bytes on each side; a multiple of 512 (the caching allocator's granule)
PATTERN = 0xFF
assert GUARD % 512 == 0

_HERE = os.path.abspath(__file__)
_ZERO_FILLED = (_torch.uint8, _torch.int8, _torch.int16, _torch.int32, _torch.int64, _torch.bool)


def _call_site() -> str:
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})"


def _shape(size) -> tuple:
    """the shape of ``empty(2, 3)``, ``empty((2, 3))``, ``empty([2, 3])``, ``empty(torch.Size(...))``, ``empty(5)`` and ``empty(())``"""
    if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
        size = size[0]
    return tuple(int(s) for s in size)


class Record:
    __slots__ = ("parent", "nbytes", "site", "shape", "dtype", "kind")

    def __init__(self, parent, nbytes, site, shape, dtype, kind):
        self.parent, self.nbytes, self.site, self.shape, self.dtype, self.kind = parent, nbytes, site, shape, dtype, kind

    def describe(self) -> str:
        return f"{self.kind} {self.shape} {self.dtype} on {self.parent.device} from {self.site}"


class GuardedTorch:
    def __init__(self, guard: int = GUARD):
        assert guard > 0 and guard % 512 == 0, guard
        self.guard = int(guard)
        self.records = []           # every parent buffer stays alive: its guards are checked, its address is not handed out again
        self.guarded = 0            # allocations that went through the replaced functions
        self.placed = 0             # inputs copied in by place()

    def __getattr__(self, name):    # everything that is not replaced below: the real torch
        return getattr(_torch, name)

    # ------------------------------------------------------------------ the one allocation
    def _alloc(self, shape, dtype, device, kind: str, fill):
        """``fill``: None = the policy of ``empty`` (0xFF for floating types, zeros for the rest), else the value asked for"""
        dtype = _torch.get_default_dtype() if dtype is None else dtype
        shape = tuple(int(s) for s in shape)
        assert all(s >= 0 for s in shape), shape
        numel = 1
        for s in shape:
            numel *= s
        item = _torch.empty((), dtype=dtype).element_size()
        nbytes = numel * item
        G = self.guard
        parent = _torch.empty(G + nbytes + G, dtype=_torch.uint8, device=device)
        parent.fill_(PATTERN)
        inner = parent[G:G + nbytes].view(dtype).view(shape)
        if fill is None:
            if dtype in _ZERO_FILLED:
                inner.zero_()
        else:
            inner.fill_(fill)
        self.records.append(Record(parent, nbytes, _call_site(), shape, dtype, kind))
        return inner

    def _new(self, size, kw, kind, fill):
        kw = dict(kw)
        dtype, device = kw.pop("dtype", None), kw.pop("device", None)
        if kw.get("requires_grad") is False:
            del kw["requires_grad"]
        assert not kw, f"guarded torch.{kind}: unsupported arguments {sorted(kw)}"
        self.guarded += 1
        return self._alloc(_shape(size), dtype, device, kind, fill)

    def _like(self, t, kw, kind, fill):
        kw = dict(kw)
        dtype, device = kw.pop("dtype", None), kw.pop("device", None)
        kw.pop("memory_format", None)       # the copy is contiguous (the wrappers only mirror contiguous tensors)
        assert not kw, f"guarded torch.{kind}: unsupported arguments {sorted(kw)}"
        self.guarded += 1
        return self._alloc(t.shape, t.dtype if dtype is None else dtype, t.device if device is None else device, kind, fill)

    # ------------------------------------------------------------------ torch's allocating functions
    def empty(self, *size, **kw):
        return self._new(size, kw, "empty", None)

    def zeros(self, *size, **kw):
        return self._new(size, kw, "zeros", 0)

    def ones(self, *size, **kw):
        return self._new(size, kw, "ones", 1)

    def full(self, size, fill_value, **kw):
        if kw.get("dtype") is None:         # torch's inference: bool -> bool, int -> int64, float -> the default dtype
            kw["dtype"] = (_torch.bool if isinstance(fill_value, bool) else _torch.int64 if isinstance(fill_value, int)
                           else _torch.get_default_dtype())
        return self._new((size,), kw, "full", fill_value)

    def empty_like(self, t, **kw):
        return self._like(t, kw, "empty_like", None)

    def zeros_like(self, t, **kw):
        return self._like(t, kw, "zeros_like", 0)

    def ones_like(self, t, **kw):
        return self._like(t, kw, "ones_like", 1)

    def full_like(self, t, fill_value, **kw):
        return self._like(t, kw, "full_like", fill_value)

    # ------------------------------------------------------------------ the test's side
    def place(self, t, device=None):
        """a contiguous copy of ``t`` (on ``device``, default: where it lives) between guards; None stays None"""
        if t is None:
            return None
        self.placed += 1
        out = self._alloc(t.shape, t.dtype, t.device if device is None else device, "place", 0)
        out.copy_(t)
        return out

    def damage(self):
        """[(record, 'low' | 'high', first, last)]: the damaged guards, offsets in bytes relative to the inner region"""
        self._synchronize()
        found = []
        G = self.guard
        for r in self.records:
            for which, band, base in (("low", r.parent[:G], -G), ("high", r.parent[G + r.nbytes:], r.nbytes)):
                if bool((band == PATTERN).all()):
                    continue
                bad = (band != PATTERN).nonzero().reshape(-1)
                found.append((r, which, base + int(bad[0]), base + int(bad[-1])))
        return found

    def check(self) -> None:
        found = self.damage()
        if found:
            lines = [f"  {r.describe()}: {which} guard damaged, bytes {first} .. {last} relative to the tensor's {r.nbytes} bytes"
                     for r, which, first, last in found]
            raise AssertionError(f"{len(found)} guard band(s) damaged among {len(self.records)} buffers:\n" + "\n".join(lines))

    def _synchronize(self) -> None:
        for d in {r.parent.device for r in self.records if r.parent.is_cuda}:
            _torch.cuda.synchronize(d)

    def snapshot(self):
        """a copy of every byte of every buffer (guards and inner region), for ``changed``"""
        self._synchronize()
        return [r.parent.clone() for r in self.records]

    def changed(self, snapshot):
        """descriptions of the buffers of ``snapshot`` that hold other bytes now (buffers made since are not looked at)"""
        self._synchronize()
        out = []
        for r, old in zip(self.records, snapshot):
            if not _torch.equal(r.parent, old):
                bad = (r.parent != old).nonzero().reshape(-1) - self.guard
                out.append(f"{r.describe()}: bytes {int(bad[0])} .. {int(bad[-1])} relative to the tensor's {r.nbytes} bytes")
        return out

    def install(self, monkeypatch, *modules) -> "GuardedTorch":
        """``monkeypatch.setattr(module, "torch", self)`` for every module: undone when the test ends"""
        for m in modules:
            assert getattr(m, "torch") is _torch or isinstance(getattr(m, "torch"), GuardedTorch), m
            monkeypatch.setattr(m, "torch", self)
        return self


def untouched(t) -> bool:
    """every byte of a floating ``empty`` tensor from a GuardedTorch still holds the fill"""
    return bool((t.contiguous().view(-1).view(_torch.uint8) == PATTERN).all())
