"""Device memory of EXACTLY the size a call asked for, between two guard zones, with hostile contents beforehand.

The library allocates nothing: every workspace, scratch and output is lent by the caller (include/iq.h).  Two promises follow -
a result never depends on what the lent memory held before, and a call never writes outside the size its ``*_bytes`` function
(or the wrapper's own formula) named.  ``workspace.ensure`` hands out memory of AT LEAST the size and keeps it across calls, and
``torch.empty`` recycles blocks of earlier calls and rounds sizes up, so neither promise can be seen to break from the ordinary
suite.  Here every allocation is one uint8 buffer of GUARD + nbytes + GUARD bytes: the guards hold 0xA5 and are compared
afterwards, the body - the exact ``nbytes`` slice - is filled by a *fill* before the call sees it.  GUARD is 4 MiB, a multiple of
256, so the body keeps the base alignment that the library's carving of a workspace assumes.

Why these three fills and no other.  A hostile fill turns a latent read-before-write of an INDEX into an address.
  ZERO   what a fresh process usually sees: the baseline.
  ONES   0xFF bytes: every float a NaN, every signed integer -1, every unsigned one its maximum.  A stale index of -1 points one
         row in front of its array; the front guard absorbs that, because no row stride here approaches 4 MiB.  But -1 loses
         every signed max merge, so ONES alone cannot see a missing zero-initialisation under ``atomicMax``.
  STALE  the bytes a *donor* call - the same route on the same shape, other inputs and weights - left in its buffers, allocation
         by allocation.  Its indices are valid for this shape, and its activations are realistic positive values: those are what
         defeats a missing zero-initialisation under a signed max merge.
No positive byte pattern (0x7F, 0x55, ...) is offered, on purpose: any bit pattern that is a large positive float is also an int32
near 10^9, and a stale index of that size leaves the allocation - a fault on a shared machine instead of a failed assertion.

``guarded_workspaces`` replaces ``workspace.ensure`` (engines reach it as a module attribute), ``guarded_empty`` installs a thin
proxy as the module global ``torch`` of the package modules that call ``torch.empty`` for a device buffer (``PATCHED_MODULES``);
``torch.empty`` itself is not touched.  Both record their buffers in call order into one ``Recording`` and check every guard on
exit.  A STALE fill replays a donor ``Recording``: allocation i of the recipient run receives the bytes of allocation i of the
donor run, and count and sizes must agree.

The classes take a device, so tests/test_guarded_alloc_cpu.py shows on CPU tensors that they catch what they claim.  Importing this
module touches no GPU.  Not collected by pytest (no test_ prefix)."""
import contextlib
import importlib

import torch

GUARD = 4 << 20
GUARD_BYTE = 0xA5
assert GUARD % 256 == 0

PACKAGE = "interpret_quality_amd"
# the package modules whose ``torch.empty`` makes a device buffer that the library reads or writes
PATCHED_MODULES = ("hip_ops", "engine", "pointnet", "pointconv", "wide", "wide_kernelshap", "final_common")


class GuardError(AssertionError):
    pass


class Guarded:
    """``body``: exactly ``nbytes`` uint8 on ``device``, filled by ``fill``, between two guards of GUARD bytes of 0xA5."""

    def __init__(self, nbytes, fill, device, label=""):
        self.nbytes, self.label = int(nbytes), label
        assert self.nbytes >= 0
        self.buf = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device=device)
        self.buf[:GUARD].fill_(GUARD_BYTE)
        self.buf[GUARD + self.nbytes:].fill_(GUARD_BYTE)
        self.body = self.buf[GUARD:GUARD + self.nbytes]
        fill(self.body)

    def guards(self):
        return (("front", self.buf[:GUARD]), ("tail", self.buf[GUARD + self.nbytes:]))

    def check(self):
        """Synchronises; GuardError naming the side and the first changed offset (front: counted from the start of the guard, so
        GUARD - 1 is the byte in front of the body; tail: 0 is the byte behind it)."""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        for side, g in self.guards():
            changed = g != GUARD_BYTE
            if bool(changed.any()):
                off = int(changed.nonzero()[0, 0])
                raise GuardError("%s guard of %s (%d bytes) changed at offset %d of %d: 0x%02x" % (
                    side, self.label or "a buffer", self.nbytes, off, GUARD, int(g[off])))


class Recording(list):
    """The Guarded buffers of one run in call order; ``workspaces``: those that ``guarded_workspaces`` handed to an engine."""

    def __init__(self):
        super().__init__()
        self.workspaces = []

    def sizes(self):
        return [g.nbytes for g in self]

    def check(self):
        for g in self:
            g.check()


def ZERO(body):
    body.zero_()


def ONES(body):
    body.fill_(0xFF)


class STALE:
    """The bytes a donor call left: ``donor`` is a Guarded (or a tensor of bytes) for one buffer, or a Recording replayed in
    order - application i copies the body of donor allocation i, whose size must be this allocation's.  ``finish`` asserts
    that every donor buffer was used."""

    def __init__(self, donor):
        self.donors = list(donor) if isinstance(donor, (list, tuple)) else [donor]
        self.used = 0

    def __call__(self, body):
        assert self.used < len(self.donors), "the recipient run allocates more than the donor's %d buffers" % len(self.donors)
        d = self.donors[self.used]
        src = d.body if isinstance(d, Guarded) else d.reshape(-1).view(torch.uint8)
        assert src.numel() == body.numel(), "allocation %d: the donor's buffer has %d bytes, this one %d" % (
            self.used, src.numel(), body.numel())
        body.copy_(src)
        self.used += 1

    def finish(self):
        assert self.used == len(self.donors), "the recipient run made %d allocations, the donor %d" % (self.used, len(self.donors))


def _finish(fill, rec):
    rec.check()
    if isinstance(fill, STALE):
        fill.finish()


@contextlib.contextmanager
def guarded_workspaces(fill, rec=None, check=True):
    """``workspace.ensure`` replaced: every engine call gets a FRESH Guarded body of exactly the size asked, after
    ``eng.workspace_replaced()``; ``eng._ws`` is that body.  Yields the Recording; on a clean exit every guard is checked
    (``check=False``: the caller checks a Recording shared with ``guarded_empty``).  The engines are left without a workspace."""
    workspace = importlib.import_module(PACKAGE + ".workspace")
    rec = Recording() if rec is None else rec
    engines = []

    def ensure(eng, nbytes):
        eng._ws = None
        eng.workspace_replaced()
        g = Guarded(nbytes, fill, eng.device, "workspace %d of %s" % (len(rec.workspaces), type(eng).__name__))
        rec.append(g)
        rec.workspaces.append(g)
        if not any(e is eng for e in engines):
            engines.append(eng)
        eng._ws = g.body
        return eng._ws

    real = workspace.ensure
    workspace.ensure = ensure
    try:
        yield rec
    finally:
        workspace.ensure = real
        for eng in engines:
            eng._ws = None
            eng.workspace_replaced()
    if check:
        _finish(fill, rec)


class TorchProxy:
    """Forwards everything to ``torch``, except that ``empty(..., device=<a device of device_type>)`` returns a view of a Guarded
    body of exactly numel * itemsize bytes."""

    def __init__(self, fill, rec, device_type):
        self._fill, self._rec, self._device_type = fill, rec, device_type

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        device = kw.get("device")
        if device is None or set(kw) - {"dtype", "device"} or torch.device(device).type != self._device_type:
            return torch.empty(*size, **kw)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        numel = 1
        for d in shape:
            numel *= int(d)
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        g = Guarded(nbytes, self._fill, device, "torch.empty %d: %s %s" % (len(self._rec), tuple(shape), dtype))
        self._rec.append(g)
        return g.body.view(dtype).view(shape)


@contextlib.contextmanager
def guarded_empty(fill, rec=None, check=True, device_type="cuda"):
    """The module global ``torch`` of every PATCHED_MODULES module replaced by a TorchProxy.  Yields the Recording; on a clean exit
    every guard is checked (``check=False``: the caller does)."""
    rec = Recording() if rec is None else rec
    proxy = TorchProxy(fill, rec, device_type)
    mods = [importlib.import_module("%s.%s" % (PACKAGE, m)) for m in PATCHED_MODULES]
    saved = [m.torch for m in mods]
    assert all(s is torch for s in saved), "a module is already patched"
    for m in mods:
        m.torch = proxy
    try:
        yield rec
    finally:
        for m, s in zip(mods, saved):
            m.torch = s
    if check:
        _finish(fill, rec)


@contextlib.contextmanager
def guarded(fill, device_type="cuda"):
    """``guarded_workspaces`` and ``guarded_empty`` together on one Recording in call order, which a STALE fill of a later run
    replays; guards (and a STALE fill's count) are checked once, on a clean exit."""
    rec = Recording()
    with guarded_workspaces(fill, rec, check=False), guarded_empty(fill, rec, check=False, device_type=device_type):
        yield rec
    _finish(fill, rec)
