"""CPU: the poison helper itself (tests/poison.py) on CPU tensors, and the completeness of tests/test_stale_memory_gpu.py:
every function of ops.py that takes a workspace has a stale-memory case, and the modules under test hold no allocation idiom
the helper's torch proxy cannot see."""
import inspect
import os
import re
import types

import pytest
import torch

import poison
from mega.pytorch_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mega", "pytorch_amd")


def _module():
    """a stand-in for a package module: its own `torch` global and two allocation sites"""
    m = types.ModuleType("stale_memory_fake")
    m.torch = torch
    exec("def make(shape, dtype):\n    return torch.empty(shape, dtype=dtype)\n\n"
         "def like(x):\n    return torch.empty_like(x)\n", m.__dict__)
    return m


# ------------------------------------------------------------------------------------------------ fill patterns
def test_ones_fill_is_nan_minus_one_255_and_all_ones():
    m = _module()
    with poison.poisoned("ones", (m,)) as p:
        for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
            assert torch.isnan(m.make((3, 5), dt)).all(), dt
        for dt in (torch.int32, torch.int64):
            assert (m.make(7, dt) == -1).all(), dt
        assert (m.make((4,), torch.uint8) == 255).all()
        words = m.make((4,), torch.int64).view(torch.uint8)                 # a 64-bit mask word: every bit set
        assert (words == 255).all()
        assert torch.isnan(m.like(torch.zeros(3, 4))).all()
        assert m.make((0, 4), torch.float32).shape == (0, 4)               # an empty tensor is counted, not filled
    assert p.count == 10 and p.ws_count == 0


def test_zeros_fill_is_the_control():
    m = _module()
    with poison.poisoned("zeros", (m,)) as p:
        for dt in (torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8):
            assert not m.make((5, 3), dt).view(torch.uint8).any(), dt
    assert p.count == 5


def test_only_three_modes():
    assert poison.MODES == ("zeros", "ones", "replay")
    with pytest.raises(ValueError):
        with poison.poisoned("0x7f", (_module(),)):
            pass


def test_ops_is_poisoned_through_its_torch_global_and_its_ws():
    real_ws = ops._ws
    with poison.poisoned("ones") as p:                                     # default: modules = (ops,)
        assert ops.torch is not torch and ops._ws is not real_ws
        t = ops.torch.empty((2, 3), dtype=torch.bfloat16)
        assert torch.isnan(t).all() and isinstance(t, ops.torch.Tensor)
        assert ops.torch.float32 is torch.float32 and ops.torch.cuda is torch.cuda      # everything else forwards
        w = ops._ws(100, "cpu")
        assert w.dtype == torch.uint8 and w.numel() == 100 and (w == 255).all()
        assert (ops.torch.empty(4, dtype=torch.int32) == -1).all()
    assert p.count == 3 and p.ws_count == 1 and p.nbytes == 3 * 256
    assert ops.torch is torch and ops._ws is real_ws


# ------------------------------------------------------------------------------------------------ replay
def test_replay_returns_the_same_addresses_after_reset():
    m = _module()
    with poison.poisoned("replay", (m,), slab_bytes=4096, device="cpu") as p:
        a = m.make((3, 5), torch.float32)
        b = m.make(7, torch.int64)
        c = m.like(torch.zeros(2, 2, dtype=torch.bfloat16))
        ptrs = [t.data_ptr() for t in (a, b, c)]
        assert all(q % poison.ALIGN == 0 for q in ptrs) and ptrs[1] - ptrs[0] == 256 and ptrs[2] - ptrs[1] == 256
        assert a.shape == (3, 5) and b.dtype == torch.int64 and c.dtype == torch.bfloat16 and c.shape == (2, 2)
        a.fill_(7.0)
        b.fill_(41)
        p.reset()
        a2 = m.make((2, 4), torch.float32)                                 # another problem on the same bytes
        b2 = m.make(7, torch.int64)
        assert a2.data_ptr() == ptrs[0] and b2.data_ptr() == ptrs[1]
        assert (a2 == 7.0).all() and (b2 == 41).all()                      # ... which still hold the previous call's values
    assert p.count == 5


def test_replay_raises_when_the_slab_is_exhausted():
    m = _module()
    with poison.poisoned("replay", (m,), slab_bytes=1024, device="cpu") as p:
        m.make(256, torch.uint8)
        m.make(192, torch.float32)                                         # 768 bytes: the slab is full
        with pytest.raises(MemoryError):
            m.make(1, torch.uint8)
        p.reset()
        with pytest.raises(MemoryError):
            m.make(1025, torch.uint8)
        assert m.make(1024, torch.uint8).numel() == 1024
    with pytest.raises(ValueError):
        with poison.poisoned("replay", (m,)):                              # no slab size: an error, not torch.empty
            pass


def test_replay_refuses_another_device_and_unknown_keywords():
    m = _module()
    with poison.poisoned("replay", (m,), slab_bytes=1024, device="cpu"):
        with pytest.raises(RuntimeError):
            m.torch.empty(4, dtype=torch.uint8, device="meta")
        with pytest.raises(TypeError):
            m.torch.empty(4, dtype=torch.uint8, pin_memory=True)


# ------------------------------------------------------------------------------------------------ restore
def test_modules_are_restored_on_exit_and_after_an_exception():
    m = _module()
    real_ws = ops._ws
    with poison.poisoned("zeros", (m, ops)):
        assert m.torch is not torch
    assert m.torch is torch and ops.torch is torch and ops._ws is real_ws
    with pytest.raises(KeyError):
        with poison.poisoned("ones", (m, ops)):
            raise KeyError("inside")
    assert m.torch is torch and ops.torch is torch and ops._ws is real_ws
    with poison.poisoned("ones", (m,)):
        with pytest.raises(RuntimeError):                                  # nesting would restore the wrong object
            with poison.poisoned("zeros", (ops, m)):
                pass
        assert ops.torch is torch                                          # (the half-entered inner context undid itself)
    assert m.torch is torch


# ------------------------------------------------------------------------------------------------ completeness
def _ws_functions():
    """names of the functions of ops.py whose source calls _ws( -- read from the file, not from the imported module, whose
    functions other tests replace with their CPU twins"""
    import ast
    with open(os.path.join(PKG, "ops.py")) as f:
        src = f.read()
    return sorted(n.name for n in ast.parse(src).body
                  if isinstance(n, ast.FunctionDef) and n.name != "_ws" and "_ws(" in ast.get_source_segment(src, n))


def test_every_workspace_operation_has_a_stale_memory_case():
    import test_stale_memory_gpu as g
    fns = _ws_functions()
    assert len(fns) >= 15 and "nms" in fns and "conv2d_nhwc" in fns
    missing = [f for f in fns if f not in g.WS_OPS]
    assert not missing, "ops.%s take a workspace but tests/test_stale_memory_gpu.py has no case for them (WS_OPS)" % missing
    stale = [f for f in g.WS_OPS if f not in fns]
    assert not stale, "WS_OPS names %s, which take no workspace (any more)" % stale
    src = inspect.getsource(g)
    callers = {"_merge_setup": ("bbox_aug_merge", "soft_merge"), "conv2d_sp": ("conv2d_sp", "linear_sp"),
               "tubelet_match": ("track_eval.run",), "vid_eval_ap": ("match_and_ap",), "seq_nms": ("seq_nms.run",),
               "link_tracks": ("tracks.run",), "motion_iou": ("motion_iou.run",)}
    for f, test in g.WS_OPS.items():
        assert callable(getattr(g, test, None)), "WS_OPS[%r] names %r, which is no test of the file" % (f, test)
        for call in callers.get(f, (f,)):
            assert re.search(r"\b%s\(" % re.escape(call), src), "%s is never called in tests/test_stale_memory_gpu.py" % call


def test_no_allocation_idiom_the_proxy_cannot_see():
    import test_stale_memory_gpu as g
    hidden = re.compile(r"new_empty|empty_strided|torch\.Tensor\(|\.new\(")
    found = []
    for name in g.MODULE_NAMES:
        with open(os.path.join(PKG, name + ".py")) as f:
            for i, line in enumerate(f, 1):
                if hidden.search(line):
                    found.append("%s.py:%d: %s" % (name, i, line.strip()))
    assert not found, "allocations the poison proxy cannot see (use torch.empty, or extend tests/poison.py):\n" + "\n".join(found)


def test_the_case_inputs_build_on_the_host():
    """the seeded inputs the GPU file picks by search meet their margins (box_boundary_cases' rule) and its size claims hold"""
    import test_stale_memory_gpu as g
    for form, specs in g.RPN_STALE.items():
        frames = g._rpn_frames(form)
        assert len(frames) == 2 and all(c.pre == specs[0].k and c.post == 300 for c in frames)
        assert min(c.reference()[0].shape[0] for c in frames) < 300        # a frame whose count stays below post_nms
    imgs = g._post_images()
    D = [c.facts["D"] for c in imgs]
    assert [c.nprop for c in imgs] == [70, 33] and D[0] > g.POST_MAX_DET > D[1] > 0, D
    for c in imgs:
        assert not bool((c.reference()[2] == g.POST_DEAD_CLASS).any())
    frames, sizes, flips = g._merge_frames("B")
    assert len(frames) == 2 and len(frames[0]) == 2 and frames[0][0][1].shape == (2, 40)
