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
