"""Stale-memory poisoning for the wrappers' allocations (tests/test_stale_memory*.py).

Every op in mega/pytorch_amd/ops.py takes its workspace from ops._ws() and almost every output from torch.empty /
torch.empty_like: uninitialised bytes.  In a short test process those bytes are usually fresh zero pages; in the clip engines
they are the previous step-batch's values.  `poisoned(mode, modules)` makes the difference visible: for its duration the
`torch` global of each named module is a forwarding proxy whose `empty` / `empty_like` fill what they return, and `ops._ws`
does the same.  A kernel whose result is a function of its inputs alone gives the same bits under every mode.

modes
  zeros    fill 0x00: the control (what a fresh process effectively sees)
  ones     fill 0xFF: NaN in f32 / bf16 / f16 / f64, -1 in i32 / i64, 255 in u8 flags, all-ones mask words
  replay   a bump allocator over ONE preallocated slab (256-byte aligned offsets); reset() rewinds it, so the next call's
           allocations land on the previous call's bytes -- the engines' situation.  Raises MemoryError when the slab is
           exhausted; never falls back to torch.empty.  Results are views of the slab: copy them out before the next reset().

No other byte pattern is offered on purpose: 0x7F and the like turn a stale count into a huge positive number, and the aim is
to detect a dependence on prior memory, not to drive a latent one out of bounds.

Not for use inside a hipGraph capture (the fills are extra launches on the capturing stream).

`guarded(modules, slab_bytes, device, guard_bytes, polarity)` (tests/test_guard_bands*.py) is the mirror image: the same slab
allocator with a guard band before and after every allocation, for the kernel that WRITES bytes it does not own.  It is an
entry point of its own, not a fourth mode.
"""
import contextlib

import torch as _torch

MODES = ("zeros", "ones", "replay")
ALIGN = 256
_FILL = {"zeros": 0x00, "ones": 0xFF}


def _shape_of(args, kwargs):
    """the size argument of torch.empty: empty(2, 3), empty((2, 3)), empty(torch.Size), empty(size=...)"""
    if "size" in kwargs:
        size = kwargs["size"]
    elif len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
        size = args[0]
    else:
        size = args
    return tuple(int(s) for s in size)


class Poison(object):
    """The state behind poisoned(): fills and counts.  count = allocations filled (empty + empty_like + _ws), ws_count = those
    that came through _ws, nbytes = the bytes they asked for, each rounded up to ALIGN (what a replay slab must hold)."""

    def __init__(self, mode, slab_bytes=0, device=None):
        if mode not in MODES:
            raise ValueError("poison mode %r, not one of %s" % (mode, MODES))
        self.mode = mode
        self.count = 0
        self.ws_count = 0
        self.nbytes = 0
        self.slab = None
        self.offset = 0
        if mode == "replay":
            if slab_bytes <= 0:
                raise ValueError("replay needs slab_bytes > 0: size it from the largest case plus a margin")
            # over-allocate by ALIGN so that the first offset can be aligned whatever the allocator returned
            raw = _torch.zeros(int(slab_bytes) + ALIGN, dtype=_torch.uint8, device=device)
            lead = (-raw.data_ptr()) % ALIGN
            self.slab = raw[lead:lead + int(slab_bytes)]

    # ---- replay
    def reset(self):
        """rewind the slab: the next allocations land on the previous call's bytes (which stay as they are)"""
        self.offset = 0

    def _carve(self, shape, dtype, device):
        dtype = _torch.get_default_dtype() if dtype is None else dtype
        device = _torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = _torch.device("cuda", _torch.cuda.current_device())
        if device != self.slab.device:
            raise RuntimeError("replay slab lives on %s, allocation asked for %s" % (self.slab.device, device))
        n = 1
        for s in shape:
            n *= s
        nb = n * _torch.empty((), dtype=dtype).element_size()
        step = (nb + ALIGN - 1) // ALIGN * ALIGN
        if self.offset + step > self.slab.numel():
            raise MemoryError("replay slab exhausted: %d bytes at offset %d of %d" % (nb, self.offset, self.slab.numel()))
        t = self.slab[self.offset:self.offset + nb].view(dtype).view(shape)
        self.offset += step
        self._account(nb)
        return t

    # ---- zeros / ones
    def _fill(self, t):
        if t.numel():
            # the storage's bytes, whatever the dtype, strides or memory format of the tensor over them
            _torch.empty(0, dtype=_torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(_FILL[self.mode])
        self._account(t.numel() * t.element_size())
        return t

    def _account(self, nb):
        self.count += 1
        self.nbytes += (nb + ALIGN - 1) // ALIGN * ALIGN

    # ---- the three entry points
    def empty(self, *args, **kwargs):
        if self.mode != "replay":
            return self._fill(_torch.empty(*args, **kwargs))
        extra = set(kwargs) - {"size", "dtype", "device"}
        if extra:
            raise TypeError("replay cannot honour torch.empty(%s)" % ", ".join(sorted(extra)))
        return self._carve(_shape_of(args, kwargs), kwargs.get("dtype"), kwargs.get("device"))

    def empty_like(self, x, **kwargs):
        if self.mode != "replay":
            return self._fill(_torch.empty_like(x, **kwargs))
        extra = set(kwargs) - {"dtype", "device"}
        if extra:
            raise TypeError("replay cannot honour torch.empty_like(%s)" % ", ".join(sorted(extra)))
        return self._carve(tuple(x.shape), kwargs.get("dtype", x.dtype), kwargs.get("device", x.device))

    def ws(self, nbytes, device):
        self.ws_count += 1
        return self.empty(int(nbytes), dtype=_torch.uint8, device=device)


class TorchProxy(object):
    """Stands in for a module's `torch` global: every attribute is the real torch's, except empty / empty_like."""

    def __init__(self, poison):
        object.__setattr__(self, "_poison", poison)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    def empty(self, *args, **kwargs):
        return self._poison.empty(*args, **kwargs)

    def empty_like(self, x, **kwargs):
        return self._poison.empty_like(x, **kwargs)


def _default_modules():
    from mega.pytorch_amd import ops
    return (ops,)


@contextlib.contextmanager
def poisoned(mode, modules=None, slab_bytes=0, device=None):
    """with poisoned("ones", (ops, seq_nms)) as p: ...; p.count allocations were filled.  modules: every module whose own
    torch.empty / empty_like sites are to be poisoned (default: ops); a module with a `_ws` function of its own (ops) gets that
    replaced as well.  replay: slab_bytes on `device`, p.reset() between calls."""
    modules = _default_modules() if modules is None else tuple(modules)
    p = Poison(mode, slab_bytes, device)
    proxy = TorchProxy(p)
    saved = []
    try:
        for m in modules:
            if getattr(m, "torch", None) is not _torch:
                raise RuntimeError("%s has no `torch` global to poison (or is poisoned already)" % m.__name__)
            saved.append((m, "torch", m.torch))
            m.torch = proxy
            if "_ws" in vars(m):
                saved.append((m, "_ws", m._ws))
                m._ws = p.ws
        yield p
    finally:
        for m, name, val in reversed(saved):
            setattr(m, name, val)


# ====================================================================================================== guard bands
POLARITIES = {"ff": (0x00, 0xFF), "00": (0xFF, 0x00)}        # polarity -> (band byte, payload pre-fill)


class _Allocation(object):
    __slots__ = ("ordinal", "kind", "shape", "dtype", "site", "front", "start", "nb", "end", "host", "written")

    def describe(self):
        return "allocation #%d (%s, shape %s, %s, %d bytes) asked for at %s" % (
            self.ordinal, self.kind, tuple(self.shape), str(self.dtype).replace("torch.", ""), self.nb, self.site)


def _site(depth):
    """file:line (function) of the frame `depth` above the caller: the line of the module under test that asked"""
    import os
    import sys
    f = sys._getframe(depth + 1)
    return "%s:%d (%s)" % (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


class Guard(object):
    """The state behind guarded(): a bump allocator over ONE slab whose every allocation is

        [ front band: guard_bytes ][ payload: first byte ALIGN-aligned, exactly nb bytes ][ back band: to the next ALIGN
                                                                                           boundary + guard_bytes ]

    The back band starts at byte nb, not at the rounded-up size, and a zero-byte allocation still gets its bands.  count,
    ws_count and nbytes count as Poison's do.  allocs: one record per allocation since the last reset(); placed: (view, host
    copy) of every place()d input."""

    def __init__(self, slab_bytes, device=None, guard_bytes=65536, polarity="ff"):
        if polarity not in POLARITIES:
            raise ValueError("guard polarity %r, not one of %s" % (polarity, sorted(POLARITIES)))
        if slab_bytes <= 0:
            raise ValueError("guarded needs slab_bytes > 0: size it from the case's allocations plus their bands")
        if guard_bytes <= 0:
            raise ValueError("guard_bytes must be positive")
        self.polarity = polarity
        self.band, self.fill = POLARITIES[polarity]
        self.guard_bytes = int(guard_bytes)
        self.count = self.ws_count = self.nbytes = 0
        raw = _torch.empty(int(slab_bytes) + ALIGN, dtype=_torch.uint8, device=device)
        lead = (-raw.data_ptr()) % ALIGN
        self.slab = raw[lead:lead + int(slab_bytes)]
        self.slab.fill_(self.band)
        self.offset = 0
        self.allocs = []
        self.placed = []

    def reset(self):
        """rewind the slab and refill the bands (every byte handed out so far goes back to the band pattern)"""
        self.slab[:self.offset].fill_(self.band)
        self.offset = 0
        self.allocs = []
        self.placed = []

    # ---- carving
    def _carve(self, shape, dtype, device, kind, site, value=None):
        dtype = _torch.get_default_dtype() if dtype is None else dtype
        device = _torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = _torch.device("cuda", _torch.cuda.current_device())
        if device != self.slab.device:
            raise RuntimeError("guard slab lives on %s, allocation asked for %s" % (self.slab.device, device))
        n = 1
        for s in shape:
            n *= s
        nb = n * _torch.empty((), dtype=dtype).element_size()
        start = (self.offset + self.guard_bytes + ALIGN - 1) // ALIGN * ALIGN
        end = (start + nb + ALIGN - 1) // ALIGN * ALIGN + self.guard_bytes
        if end > self.slab.numel():
            raise MemoryError("guard slab exhausted: %d bytes (+ bands) at offset %d of %d" % (nb, self.offset, self.slab.numel()))
        a = _Allocation()
        a.ordinal, a.kind, a.shape, a.dtype, a.site = len(self.allocs), kind, tuple(shape), dtype, site
        a.front, a.start, a.nb, a.end, a.host, a.written = self.offset, start, nb, end, None, False
        self.allocs.append(a)
        self.offset = end
        t = self.slab[start:start + nb].view(dtype).view(shape)
        if nb:
            if value is None:
                self.slab[start:start + nb].fill_(self.fill)
            else:
                t.fill_(value)
        self.count += 1
        self.nbytes += (nb + ALIGN - 1) // ALIGN * ALIGN
        return t

    def _foreign_host(self, device):
        """an allocation on the host while the slab is on a device (a weight-packing buffer, a pinned read-back buffer): no
        kernel can write it, so it is forwarded to torch.  Any other device than the slab's is an error."""
        return _torch.device("cpu" if device is None else device).type == "cpu" and self.slab.device.type != "cpu"

    # ---- the allocation entry points
    def empty(self, *args, _site_=None, _kind="empty", _value=None, **kwargs):
        if _kind == "empty" and self._foreign_host(kwargs.get("device")):
            return _torch.empty(*args, **kwargs)
        extra = set(kwargs) - {"size", "dtype", "device"}
        if extra:
            raise TypeError("guarded cannot honour torch.%s(%s)" % (_kind, ", ".join(sorted(extra))))
        return self._carve(_shape_of(args, kwargs), kwargs.get("dtype"), kwargs.get("device"), _kind, _site_ or _site(1), _value)

    def empty_like(self, x, _site_=None, _kind="empty_like", _value=None, **kwargs):
        if _kind == "empty_like" and self._foreign_host(kwargs.get("device", x.device)):
            return _torch.empty_like(x, **kwargs)
        extra = set(kwargs) - {"dtype", "device"}
        if extra:
            raise TypeError("guarded cannot honour torch.%s(%s)" % (_kind, ", ".join(sorted(extra))))
        return self._carve(tuple(x.shape), kwargs.get("dtype", x.dtype), kwargs.get("device", x.device), _kind, _site_ or _site(1), _value)

    def zeros(self, *args, _site_=None, **kwargs):
        if self._foreign_host(kwargs.get("device")):
            return _torch.zeros(*args, **kwargs)
        return self.empty(*args, _site_=_site_ or _site(1), _kind="zeros", _value=0, **kwargs)

    def zeros_like(self, x, _site_=None, **kwargs):
        if self._foreign_host(kwargs.get("device", x.device)):
            return _torch.zeros_like(x, **kwargs)
        return self.empty_like(x, _site_=_site_ or _site(1), _kind="zeros_like", _value=0, **kwargs)

    def full(self, size, fill_value, _site_=None, **kwargs):
        if self._foreign_host(kwargs.get("device")):
            return _torch.full(size, fill_value, **kwargs)
        if kwargs.get("dtype") is None:
            kwargs["dtype"] = (_torch.bool if isinstance(fill_value, bool) else _torch.int64 if isinstance(fill_value, int)
                               else _torch.get_default_dtype())
        size = (size,) if isinstance(size, int) else size
        return self.empty(size, _site_=_site_ or _site(1), _kind="full", _value=fill_value, **kwargs)

    def ws(self, nbytes, device):
        self.ws_count += 1
        return self.empty(int(nbytes), dtype=_torch.uint8, device=device, _site_=_site(1), _kind="_ws")

    # ---- inputs
    def place(self, t, device=None):
        """copy `t` (host or device) into a guarded allocation of its exact byte size -> the view.  The input then ends where a
        band begins; check() also verifies that it still holds what was placed, unless writes() registered it."""
        src = t.detach().contiguous()
        view = self._carve(tuple(src.shape), src.dtype, self.slab.device if device is None else device, "placed", _site(1))
        view.copy_(src)
        host = src.cpu().clone()
        self.allocs[-1].host = host
        self.placed.append((view, host))
        return view

    def _owner(self, t):
        at = t.data_ptr() - self.slab.data_ptr()
        for a in self.allocs:
            if a.start <= at < a.start + max(a.nb, 1):
                return a
        raise ValueError("writes(): the tensor is no part of an allocation of this guard")

    def writes(self, t):
        """register `t` (an allocation of this guard, or a view into one) as a documented in-place destination: check()
        does not compare it with what was placed.  Its bands are checked like everyone's."""
        self._owner(t).written = True
        return t

    # ---- the check
    def check(self):
        """after torch.cuda.synchronize(): every band still holds its pattern and every placed input its bytes"""
        if not self.allocs:
            return
        flags = []
        for a in self.allocs:
            flags.append((self.slab[a.front:a.start] != self.band).any())
            flags.append((self.slab[a.start + a.nb:a.end] != self.band).any())
        bad = _torch.stack(flags).cpu().tolist()                           # (one read-back for all the bands)
        errors = []
        for a in self.allocs:
            for which, hit in (("front", bad[2 * a.ordinal]), ("back", bad[2 * a.ordinal + 1])):
                if not hit:
                    continue
                lo, hi = (a.front, a.start) if which == "front" else (a.start + a.nb, a.end)
                raw = self.slab[lo:hi].cpu()
                at = (raw != self.band).nonzero().reshape(-1)
                base = a.start if which == "front" else a.start + a.nb
                first, last = int(at[0]) + lo - base, int(at[-1]) + lo - base
                errors.append("%s: %s band overwritten, %d bytes, first at offset %+d and last at %+d relative to the payload's %s "
                              "(polarity %s, first byte 0x%02x)" % (a.describe(), which, at.numel(), first, last,
                                                                    "start" if which == "front" else "end", self.polarity,
                                                                    int(raw[int(at[0])])))
            if a.host is not None and not a.written and a.nb:
                now = self.slab[a.start:a.start + a.nb].cpu()
                was = a.host.reshape(-1).view(_torch.uint8)
                if not _torch.equal(now, was):
                    at = (now != was).nonzero().reshape(-1)
                    errors.append("%s: a placed input was written, %d bytes, first at offset %d and last at %d of the payload" % (
                        a.describe(), at.numel(), int(at[0]), int(at[-1])))
        if errors:
            raise AssertionError("guard bands: %d finding(s)\n" % len(errors) + "\n".join(errors))


class GuardProxy(TorchProxy):
    """TorchProxy for guarded(): zeros / zeros_like / full are carved from the slab as well (ops.py makes outputs with all of
    them); each call records the line of the module under test that made it."""

    def empty(self, *args, **kwargs):
        return self._poison.empty(*args, _site_=_site(1), **kwargs)

    def empty_like(self, x, **kwargs):
        return self._poison.empty_like(x, _site_=_site(1), **kwargs)

    def zeros(self, *args, **kwargs):
        return self._poison.zeros(*args, _site_=_site(1), **kwargs)

    def zeros_like(self, x, **kwargs):
        return self._poison.zeros_like(x, _site_=_site(1), **kwargs)

    def full(self, size, fill_value, **kwargs):
        return self._poison.full(size, fill_value, _site_=_site(1), **kwargs)


@contextlib.contextmanager
def guarded(modules=None, slab_bytes=0, device=None, guard_bytes=65536, polarity="ff"):
    """with guarded((ops,), slab_bytes=n, device=dev) as p: x = p.place(x); y = ops.f(x); torch.cuda.synchronize(); p.check()

    Like `replay`, every torch.empty / empty_like / _ws of `modules` (default: ops) -- and here also zeros / zeros_like / full --
    is carved from one preallocated slab, never from torch.empty; MemoryError when the slab is exhausted.  Each allocation lies
    between two guard bands (see Guard), so a store past the last byte of an output, a workspace or a placed input lands in a
    band and check() reports it, with the allocation's ordinal, shape, dtype, kind, the line that asked for it, and the first
    and last overwritten offset.  Nothing faults: the stray bytes are inside the slab.

    polarity "ff": bands 0x00, payload pre-filled 0xFF (so the run is a `ones` run as well); "00": bands 0xFF, payload 0x00.
    zeros / full payloads hold their requested value under both.  A stray byte differs from 0x00 or from 0xFF, so running both
    polarities catches every overwritten byte under at least one.  No third pattern is offered, for the reason given above.

    guard_bytes: the width of each band.  A whole unmasked GEMM tile writes rows x ldo x element size bytes: pass at least that
    for the conv family, so that the tile lands in the band and not behind it.  p.reset() rewinds the slab and refills the bands.

    Not for use inside a hipGraph capture (the fills and the checks are extra launches on the capturing stream).  Results are
    views of the slab: copy them out before reset() or the end of the block."""
    modules = _default_modules() if modules is None else tuple(modules)
    p = Guard(slab_bytes, device, guard_bytes, polarity)
    proxy = GuardProxy(p)
    saved = []
    try:
        for m in modules:
            if getattr(m, "torch", None) is not _torch:
                raise RuntimeError("%s has no `torch` global to guard (or is poisoned already)" % m.__name__)
            saved.append((m, "torch", m.torch))
            m.torch = proxy
            if "_ws" in vars(m):
                saved.append((m, "_ws", m._ws))
                m._ws = p.ws
        yield p
    finally:
        for m, name, val in reversed(saved):
            setattr(m, name, val)
