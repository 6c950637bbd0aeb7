"""An allocation shim for the gzero wrappers: every ``torch.empty`` they make comes
back filled with a chosen byte and followed by a guard band.

    with poisoned(0xFF) as mem:        # 0xFF: ints of -1, fp16 / fp32 / fp64 NaN
        out = device.pv_forward(w, rows)
        mem.check()                    # every guard band still holds 0xA5

While the context is active the module-level name ``torch`` of gzero.device,
gzero.selfplay, gzero.arena, gzero.sgd, gzero.optim and gzero.train is a proxy that
forwards every attribute to the real torch except ``empty``.  ``empty`` allocates the
requested bytes plus ``guard_bytes``, fills the requested part with ``pattern`` (one
byte value, or "leftover" = leave what is there), fills the tail with 0xA5 and returns
the view of the requested part; its data_ptr() is the base pointer, so alignment is
what the allocator gives.  The base tensors are kept: ``check()`` (and leaving the
context) asserts that every tail is still all 0xA5 and names the allocating call site
and the first changed offset otherwise.  ``torch.zeros`` is not touched: an argument
the caller must zero is the API's business, not the library's.

``reuse=`` (another, finished context): an allocation takes the buffer the same call
site (file:line, and which visit of it) got there when it is large enough, at the same
address, with the guard moved up behind the smaller size.  With "leftover" that is how a
one-shot wrapper, which allocates its workspace inside the call, is handed the bytes a
larger call left behind.

A test helper, imported by the tests that want it; nothing here runs on its own.
"""
import contextlib
import importlib
import math
import os
import sys

import torch as _torch

GUARD_BYTE = 0xA5
LEFTOVER = "leftover"
MODULES = ("gzero.device", "gzero.selfplay", "gzero.arena", "gzero.sgd", "gzero.optim", "gzero.train")
_HERE = os.path.abspath(__file__)


class GuardError(AssertionError):
    pass


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?:0"
    return f"{f.f_code.co_filename}:{f.f_lineno}"


class _Allocation:
    __slots__ = ("base", "nbytes", "guard", "site", "key")

    def __init__(self, base, nbytes, guard, site, key):
        self.base, self.nbytes, self.guard, self.site, self.key = base, nbytes, guard, site, key

    def first_changed(self):
        """Offset past the requested bytes of the first guard byte that changed, or None."""
        tail = self.base[self.nbytes:self.nbytes + self.guard]
        bad = (tail != GUARD_BYTE).nonzero()
        return int(bad[0, 0]) if bad.numel() else None


class _TorchProxy:
    """The real torch with ``empty`` replaced."""

    def __init__(self, pool):
        self.__dict__["_pool"] = pool

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    def empty(self, *size, dtype=None, device=None, requires_grad=False, **unsupported):
        if unsupported:
            raise NotImplementedError(f"devmem: torch.empty({', '.join(unsupported)}=...) is not modelled")
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        shape = tuple(int(s) for s in size)
        dtype = _torch.get_default_dtype() if dtype is None else dtype
        numel = math.prod(shape)
        nbytes = numel * _torch.empty((), dtype=dtype).element_size()
        base = self._pool._allocate(nbytes, device, _call_site())
        view = base[:nbytes].view(dtype).view(shape)
        assert nbytes == 0 or view.data_ptr() == base.data_ptr()
        return view.requires_grad_() if requires_grad else view


class Poisoned:
    def __init__(self, pattern, guard_bytes=65536, reuse=None, modules=None):
        if pattern != LEFTOVER and not (isinstance(pattern, int) and 0 <= pattern <= 255):
            raise ValueError(f"pattern must be one byte value or {LEFTOVER!r}, not {pattern!r}")
        self.pattern = pattern
        self.guard_bytes = int(guard_bytes)
        self.allocations = []
        self.torch = _TorchProxy(self)
        self._visits = {}
        self._reuse = {a.key: a for a in reuse.allocations} if reuse is not None else {}
        self._modules = modules
        self._saved = []

    # ---- allocation
    def _allocate(self, nbytes, device, site):
        visit = self._visits.get(site, 0)
        self._visits[site] = visit + 1
        key = (site, visit)
        total = nbytes + self.guard_bytes
        old = self._reuse.get(key)
        want = _torch.device("cpu" if device is None else device)
        if old is not None and old.base.numel() >= total and old.base.device.type == want.type:
            base = old.base
        else:
            base = _torch.empty(total, dtype=_torch.uint8, device=device)
        if self.pattern != LEFTOVER:
            base[:nbytes].fill_(self.pattern)
        base[nbytes:total].fill_(GUARD_BYTE)
        self.allocations.append(_Allocation(base, nbytes, self.guard_bytes, site, key))
        return base

    # ---- the guards
    def check(self):
        for a in self.allocations:
            off = a.first_changed()
            if off is not None:
                raise GuardError(f"guard band changed: the {a.nbytes}-byte buffer allocated at {a.site} was "
                                 f"overrun, first changed byte at offset {a.nbytes + off} "
                                 f"({off} past its end)")

    def reused(self, site_suffix=None):
        """Allocations that took their buffer from ``reuse`` (all, or those of one site)."""
        return [a for a in self.allocations if a.key in self._reuse and a.base is self._reuse[a.key].base
                and (site_suffix is None or a.site.endswith(site_suffix))]

    # ---- patching
    def __enter__(self):
        mods = self._modules
        if mods is None:
            mods = [importlib.import_module(m) for m in MODULES]
        for m in mods:
            self._saved.append((m, m.torch))
            m.torch = self.torch
        return self

    def __exit__(self, exc_type, exc, tb):
        for m, real in reversed(self._saved):
            m.torch = real
        self._saved = []
        if exc_type is None:
            self.check()
        return False


@contextlib.contextmanager
def poisoned(pattern, guard_bytes=65536, reuse=None, modules=None):
    with Poisoned(pattern, guard_bytes, reuse, modules) as mem:
        yield mem
