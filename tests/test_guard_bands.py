"""CPU: the guarded allocator of tests/poison.py on CPU tensors -- faults planted with plain tensor writes through the slab's
uint8 view are caught and reported with the right allocation and offset -- and the completeness of
tests/test_guard_bands_gpu.py: every function of ops.py that launches a kernel (its source contains a _call() runs fenced."""
import ast
import os
import re
import types

import pytest
import torch

import poison
from mega.pytorch_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mega", "pytorch_amd")
G = 512                                  # the band width of these tests


def _module():
    """a stand-in for a package module: its own `torch` global, its own _ws, and one site of every allocation idiom"""
    m = types.ModuleType("guard_bands_fake")
    m.torch = torch
    exec("def _ws(nbytes, device):\n    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)\n\n"
         "def make(shape, dtype):\n    return torch.empty(shape, dtype=dtype)\n\n"
         "def like(x):\n    return torch.empty_like(x)\n\n"
         "def zeros(shape, dtype):\n    return torch.zeros(shape, dtype=dtype)\n\n"
         "def zeros_like(x):\n    return torch.zeros_like(x)\n\n"
         "def full(shape, v, dtype):\n    return torch.full(shape, v, dtype=dtype)\n\n"
         "def work(nbytes):\n    return _ws(nbytes, 'cpu')\n", m.__dict__)
    return m


def _guarded(m, polarity="ff", slab=1 << 16, guard=G):
    return poison.guarded((m,), slab_bytes=slab, device="cpu", guard_bytes=guard, polarity=polarity)


def _at(p, t):
    """offset of a tensor's first byte in the slab"""
    return t.data_ptr() - p.slab.data_ptr()


def _fails(p):
    with pytest.raises(AssertionError) as e:
        p.check()
    return str(e.value)


# ------------------------------------------------------------------------------------------------ layout and fill
@pytest.mark.parametrize("polarity", ["ff", "00"])
def test_layout_alignment_and_fill(polarity):
    m = _module()
    band, fill = {"ff": (0, 255), "00": (255, 0)}[polarity]
    with _guarded(m, polarity) as p:
        a = m.make((3, 50), torch.uint8)                                   # 150 bytes: ends on no 16-byte boundary
        b = m.make((0, 4), torch.float32)                                  # zero bytes: bands all the same
        c = m.like(torch.zeros(5, 7, dtype=torch.bfloat16))
        z = m.zeros((5,), torch.int32)
        zl = m.zeros_like(torch.ones(3, dtype=torch.float64))
        f = m.full((7,), -1, torch.int64)
        w = m.work(4950)
        ts = (a, b, c, z, zl, f, w)
        assert [x.kind for x in p.allocs] == ["empty", "empty", "empty_like", "zeros", "zeros_like", "full", "_ws"]
        assert all(_at(p, t) % poison.ALIGN == 0 for t in ts if t.numel())       # (an empty tensor has no address)
        prev_end = 0
        for t, rec in zip(ts, p.allocs):
            nb = t.numel() * t.element_size()
            assert rec.nb == nb and rec.start % poison.ALIGN == 0 and rec.start == (_at(p, t) if nb else rec.start) and rec.front == prev_end
            assert rec.start - rec.front >= G                              # the front band
            assert rec.end == (rec.start + nb + 255) // 256 * 256 + G      # the back band: from byte nb to the boundary + G
            assert bool((p.slab[rec.front:rec.start] == band).all()) and bool((p.slab[rec.start + nb:rec.end] == band).all())
            prev_end = rec.end
        assert bool((a == fill).all()) and bool((w == fill).all()) and bool((c.view(torch.uint8) == fill).all())
        assert not bool(z.any()) and not bool(zl.any()) and bool((f == -1).all())       # the requested value, both polarities
        assert b.shape == (0, 4) and c.shape == (5, 7) and c.dtype == torch.bfloat16 and zl.dtype == torch.float64
        assert "test_guard_bands" not in p.allocs[0].site and "(make)" in p.allocs[0].site and "(work)" in p.allocs[6].site
        p.check()
    assert p.count == 7 and p.ws_count == 1 and p.nbytes == 256 * (1 + 0 + 1 + 1 + 1 + 1) + 5120


def test_reset_rewinds_and_refills():
    m = _module()
    with _guarded(m) as p:
        a = m.make(100, torch.uint8)
        at = _at(p, a)
        p.slab[at + 100] = 7
        assert "allocation #0" in _fails(p)
        p.reset()
        assert p.allocs == [] and p.placed == []
        b = m.make(10, torch.uint8)
        assert _at(p, b) == at and bool((p.slab[at + 10:at + 256 + G] == 0).all())
        p.check()


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("kind", ["empty", "_ws"])
@pytest.mark.parametrize("fault", ["payload end + 0", "last byte of the back band", "front band end - 1"])
def test_a_planted_byte_is_caught_with_ordinal_and_offset(kind, fault):
    m = _module()
    with _guarded(m) as p:
        m.make(16, torch.uint8)
        t = m.make((3, 50), torch.uint8) if kind == "empty" else m.work(150)      # 150 bytes: no multiple of 16
        m.make(16, torch.uint8)
        assert t.numel() % 16 != 0
        rec, at = p.allocs[1], _at(p, t)
        p.check()
        where, band, off = {"payload end + 0": (at + 150, "back", 0),
                            "last byte of the back band": (rec.end - 1, "back", rec.end - 1 - (at + 150)),
                            "front band end - 1": (at - 1, "front", -1)}[fault]
        p.slab[where] = 0x5A
        msg = _fails(p)
        assert "1 finding" in msg and "allocation #1 " in msg and "allocation #0" not in msg and "allocation #2" not in msg
        assert "(%s, shape %s, uint8, 150 bytes)" % (kind, (3, 50) if kind == "empty" else (150,)) in msg
        assert "(%s)" % ("make" if kind == "empty" else "work") in msg                  # the line that asked for it
        assert "%s band overwritten, 1 bytes, first at offset %+d and last at %+d" % (band, off, off) in msg
        assert "payload's %s" % ("end" if band == "back" else "start") in msg and "0x5a" in msg
        p.slab[where] = 0
        p.check()


def test_an_extent_is_reported_first_to_last():
    m = _module()
    with _guarded(m) as p:
        t = m.make(4950, torch.uint8)
        at = _at(p, t)
        p.slab[at + 4950:at + 4950 + 10] = 1                               # a 16-byte store over a 6-byte tail
        msg = _fails(p)
        assert "back band overwritten, 10 bytes, first at offset +0 and last at +9" in msg


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x3C])
def test_the_union_of_the_polarities_catches_every_byte(byte):
    """a stray byte equal to one polarity's band pattern is invisible under it and caught under the other"""
    m = _module()
    caught = {}
    for polarity in ("ff", "00"):
        with _guarded(m, polarity) as p:
            t = m.make(150, torch.uint8)
            p.slab[_at(p, t) + 150] = byte
            try:
                p.check()
                caught[polarity] = False
            except AssertionError:
                caught[polarity] = True
    assert caught["ff"] or caught["00"]
    assert caught == {0x00: {"ff": False, "00": True}, 0xFF: {"ff": True, "00": False}, 0x3C: {"ff": True, "00": True}}[byte]


# ------------------------------------------------------------------------------------------------ placed inputs
def test_a_placed_input_ends_at_its_band_and_is_compared():
    m = _module()
    with _guarded(m) as p:
        src = torch.arange(75, dtype=torch.int16).view(3, 25)
        x = p.place(src)
        y = p.place(src.t())                                               # (made contiguous)
        assert x.dtype == torch.int16 and x.shape == (3, 25) and torch.equal(x, src) and torch.equal(y, src.t())
        assert p.allocs[0].kind == "placed" and p.allocs[0].nb == 150 and _at(p, x) % 256 == 0
        assert len(p.placed) == 2 and torch.equal(p.placed[0][1], src) and p.placed[0][0] is x
        assert "test_guard_bands" in p.allocs[0].site
        p.check()
        x[1, 3] += 1
        msg = _fails(p)
        assert "allocation #0 (placed, shape (3, 25), int16, 150 bytes)" in msg and "a placed input was written, 1 bytes" in msg
        assert "first at offset 56 and last at 56" in msg
        p.writes(x[1:])                                                    # a view registers its allocation
        p.check()
        p.slab[_at(p, x) + 150] = 9                                        # ... whose bands are still checked
        assert "allocation #0" in _fails(p)
        with pytest.raises(ValueError):
            p.writes(torch.zeros(3))


# ------------------------------------------------------------------------------------------------ refusals and restore
def test_exhaustion_unknown_keyword_wrong_device_and_bad_arguments():
    m = _module()
    with _guarded(m, slab=4 * 256 + 2 * G, guard=G) as p:
        m.make(256, torch.uint8)                                           # front G, payload 256, back G
        with pytest.raises(MemoryError):
            m.make(1, torch.uint8)
        with pytest.raises(MemoryError):
            p.place(torch.zeros(1))
        p.reset()
        assert m.make(4 * 256, torch.uint8).numel() == 1024
        p.reset()
        with pytest.raises(TypeError):
            m.torch.empty(4, dtype=torch.uint8, pin_memory=True)
        with pytest.raises(TypeError):
            m.torch.zeros(4, dtype=torch.uint8, requires_grad=True)
        with pytest.raises(RuntimeError):
            m.torch.empty(4, dtype=torch.uint8, device="meta")
        with pytest.raises(RuntimeError):
            m.torch.full((4,), 1, dtype=torch.uint8, device="meta")
        with pytest.raises(AttributeError):
            m.torch.empty = None                                           # the proxy is read-only
    for kw in ({"polarity": "7f"}, {"slab_bytes": 0}, {"guard_bytes": 0}):
        with pytest.raises(ValueError):
            with poison.guarded((m,), **dict({"slab_bytes": 4096, "device": "cpu"}, **kw)):
                pass
    assert poison.MODES == ("zeros", "ones", "replay")                     # a new entry point, not a fourth mode
    assert m.torch is torch


def test_modules_are_restored_on_exit_and_after_an_exception():
    m = _module()
    real_ws, fake_ws = ops._ws, m._ws
    with poison.guarded((m, ops), slab_bytes=8192, device="cpu", guard_bytes=G) as p:
        assert m.torch is not torch and ops.torch is not torch and ops._ws is not real_ws and m._ws is not fake_ws
        w = ops._ws(100, "cpu")
        assert w.numel() == 100 and bool((w == 255).all()) and p.ws_count == 1 and "test_guard_bands" in p.allocs[0].site
        assert ops.torch.float32 is torch.float32 and ops.torch.cuda is torch.cuda
    assert m.torch is torch and ops.torch is torch and ops._ws is real_ws and m._ws is fake_ws
    with pytest.raises(KeyError):
        with poison.guarded((m, ops), slab_bytes=8192, device="cpu"):
            raise KeyError("inside")
    assert m.torch is torch and ops.torch is torch and ops._ws is real_ws and m._ws is fake_ws
    with poison.poisoned("ones", (m,)):
        with pytest.raises(RuntimeError):                                  # no nesting, with the other helper either
            with poison.guarded((ops, m), slab_bytes=8192, device="cpu"):
                pass
        assert ops.torch is torch and ops._ws is real_ws
    assert m.torch is torch


# ------------------------------------------------------------------------------------------------ completeness
def _launching_functions():
    """names of the functions of ops.py whose source contains a _call( -- read from the file, not from the imported module"""
    with open(os.path.join(PKG, "ops.py")) as f:
        src = f.read()
    return sorted(n.name for n in ast.parse(src).body
                  if isinstance(n, ast.FunctionDef) and n.name != "_call" and "_call(" in ast.get_source_segment(src, n))


def test_every_launching_wrapper_runs_fenced():
    import test_guard_bands_gpu as g
    fns = _launching_functions()
    assert len(fns) >= 53 and "conv2d_nhwc" in fns and "jpeg_reconstruct" in fns and "nms" in fns
    missing = [f for f in fns if f not in g.GUARD_OPS]
    assert not missing, "ops.%s launch kernels but tests/test_guard_bands_gpu.py runs no fenced case of them (GUARD_OPS)" % missing
    stale = [f for f in g.GUARD_OPS if f not in fns]
    assert not stale, "GUARD_OPS names %s, which launch nothing (any more)" % stale
    for f, tests in g.GUARD_OPS.items():
        for test in (tests,) if isinstance(tests, str) else tests:
            assert callable(getattr(g, test, None)) and test.startswith("test_"), \
                "GUARD_OPS[%r] names %r, which is no test of the file" % (f, test)


def test_the_fenced_modules_hold_no_allocation_idiom_the_proxy_cannot_see():
    """test_stale_memory.py's check, over the modules the guard file fences (it fences more).  The idiom list is that test's:
    the uninitialised allocations.  Tensor.new_zeros buffers (modeling, relation, fgfa and engine hold a few: zero pads and
    staging rows) are initialised where they are made and stay outside the slab, unfenced."""
    import test_guard_bands_gpu as g
    hidden = re.compile(r"new_empty|empty_strided|torch\.Tensor\(|\.new\(")
    found = []
    for name in g.MODULE_NAMES:
        with open(os.path.join(PKG, name + ".py")) as f:
            for i, line in enumerate(f, 1):
                if hidden.search(line):
                    found.append("%s.py:%d: %s" % (name, i, line.strip()))
    assert not found, "allocations the guard proxy cannot see:\n" + "\n".join(found)
