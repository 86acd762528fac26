"""-m gpu: the five position-logit kernels of csrc/relation.hip against float64 on exact box lattices
(tests/position_cases.py: the box sets, the probe / floor / straddle / seeded weights, the float64 reference and the bounds,
all derived there; tests/test_position_cases.py proves them on the CPU).

  kind         kernel                                   reached through
  precise      pos_logits_kernel<true>                  ops.position_logits(precise=True)
  mfma         pos_logits_mfma_kernel                   ops.position_logits(precise=False)  (ldp % 32 == 0, aligned rows)
  valu         pos_logits_kernel<false>                 mega_position_logits through ctypes with ldp % 4 != 0
  tiled_bf16   pos_logits_tiled_batched_kernel<bf16_t>  ops.position_logits(tiled=dtype): one problem per launch, and
  tiled_f16    pos_logits_tiled_batched_kernel<f16_t>   ops.position_logits_batched: the five shapes of a box set in one launch

Every test prints its worst error / bound (run with -s).  For the tiled kinds the check is an interval of 16-bit values
and the figure reads 1.000 whenever a stored value sits on an end of its interval, which is the rule when the interval holds
the two neighbours of the float64 logit: the probes and the floor set also print how many values the intervals hold."""
import math

import pytest
import torch

import position_cases as pc
from test_kernels_gpu import _untile_pos

pytestmark = pytest.mark.gpu

LAUNCHES = [("precise", "single"), ("valu", "single"), ("mfma", "single"), ("tiled_bf16", "single"), ("tiled_bf16", "batched"),
            ("tiled_f16", "single"), ("tiled_f16", "batched")]


def _lid(launch):
    return "%s-%s" % launch


def _ops():
    from mega.pytorch_amd import ops
    return ops


class Runner:
    """run(wg_t, bg) -> f32 [16, Nq, Nk] on the CPU for every shape of one box set through one kernel; a batched launch
    computes the five shapes at once and hands them out one by one"""

    def __init__(self, kind, mode, dev, name):
        self.kind, self.mode, self.dev, self.name = kind, mode, dev, name
        self.boxes = {s: tuple(b.to(dev).contiguous() for b in pc.box_set(name, *s)) for s in pc.SHAPES}
        self.dim_mat = pc.dim_mat().to(dev)
        self.memo = {}

    def _tiled(self, raw, Nq, Nk):
        dt = pc.TILED[self.kind]
        assert raw.dtype == dt and tuple(raw.shape) == (16, (Nk + 31) // 32, Nq, 32)
        host = raw.cpu()
        # the kernel writes whole 32-key tiles (the pad keys of the last one repeat key Nk - 1): all of it is a logit
        assert torch.isfinite(host.float()).all(), "%s %s (%d, %d): a non-finite value in a written tile" % (self.kind, self.name, Nq, Nk)
        return _untile_pos(host, Nk)

    def launch(self, wg_t, bg, shapes=None):
        """-> {shape: f32 [16, Nq, Nk] on the CPU}; a batched launch always computes the five shapes of the set"""
        ops = _ops()
        wg, b = wg_t.to(self.dev).contiguous(), bg.to(self.dev).contiguous()
        if self.mode == "batched":
            outs = ops.position_logits_batched([self.boxes[s][0] for s in pc.SHAPES], [self.boxes[s][1] for s in pc.SHAPES],
                                               wg, b, self.dim_mat, precise=False, tiled=pc.TILED[self.kind])
            return {s: self._tiled(o, *s) for s, o in zip(pc.SHAPES, outs)}
        res = {}
        for (Nq, Nk) in shapes or pc.SHAPES:
            bq, bk = self.boxes[(Nq, Nk)]
            if self.kind in pc.TILED:
                res[(Nq, Nk)] = self._tiled(ops.position_logits(bq, bk, wg, b, self.dim_mat, precise=False, tiled=pc.TILED[self.kind]), Nq, Nk)
            elif self.kind == "valu":
                from mega.pytorch_amd import _lib
                ldp = Nk + 1 if (Nk + 1) % 4 else Nk + 2         # ldp % 4 != 0: the entry cannot take the MFMA kernel
                assert ldp % 4 != 0
                out = torch.full((16, Nq, ldp), math.nan, dtype=torch.float32, device=self.dev)
                rc = _lib.load().mega_position_logits(bq.data_ptr(), bk.data_ptr(), wg.data_ptr(), b.data_ptr(), self.dim_mat.data_ptr(),
                                                      out.data_ptr(), Nq, Nk, ldp, 0, ops._stream())
                _lib.check(rc, "mega_position_logits")
                host = out.cpu()
                assert torch.isnan(host[:, :, Nk:]).all(), "pad columns written"
                res[(Nq, Nk)] = host[:, :, :Nk]
            else:
                res[(Nq, Nk)] = ops.position_logits(bq, bk, wg, b, self.dim_mat, precise=self.kind == "precise").cpu()[:, :, :Nk]
        return res

    def run_for(self, shape):
        def run(wg_t, bg):
            key = (wg_t.numpy().tobytes(), bg.numpy().tobytes()) + (() if self.mode == "batched" else shape)
            if key not in self.memo:
                self.memo[key] = self.launch(wg_t, bg, [shape])
            return self.memo[key][shape]
        return run


def _over_shapes(check, kind, mode, dev, name, **kw):
    """`check` on every shape of a set, through one Runner: a batched launch of a weight set serves all five shapes"""
    runner = Runner(kind, mode, dev, name)
    worst = (0.0, "")
    for shape in pc.SHAPES:
        ratio, what = check(kind, (name,) + shape, runner.run_for(shape), **kw)
        if ratio > worst[0]:
            worst = (ratio, "%dx%d %s" % (shape + (what,)))
    return worst


def _pinned(kind, intervals):
    """tiled kinds: how many 16-bit values the intervals hold (2 = the neighbours of a value that is not representable)"""
    if kind not in pc.TILED:
        return ""
    n = torch.cat([pc.values_in_interval(kind, lo, hi).flatten() for lo, hi in intervals]).double()
    return ", 16-bit values per interval: median %d, exactly two in %.1f %% (the values crowd round logit 0)" % (
        int(n.median()), 100.0 * (n == 2).double().mean())


# ------------------------------------------------------------------------------------------------ 1. probes
@pytest.mark.parametrize("name", pc.SETS)
@pytest.mark.parametrize("launch", LAUNCHES, ids=_lid)
def test_probes(dev, launch, name):
    """one embedding entry per head, all 64 entries, both signs: every entry within its bound of float64"""
    kind, mode = launch
    ratio, what = _over_shapes(pc.check_probes, kind, mode, dev, name)
    extra = _pinned(kind, [pc.probe_interval(kind, pc.reference(name, *s)[1], r, sg) for s in pc.SHAPES for r, sg in pc.PROBES]
                    if kind in pc.TILED else [])
    print("probes %s %s: worst error / bound %.3f at %s%s" % (_lid(launch), name, ratio, what, extra))
    assert ratio <= 1.0, (launch, ratio, what)


# ------------------------------------------------------------------------------------------------ 2. floor set
@pytest.mark.parametrize("name", pc.SETS)
@pytest.mark.parametrize("launch", LAUNCHES, ids=_lid)
def test_floor(dev, launch, name):
    """Wg = 0, 16 biases round 0: log(max(b, 0) + 1e-6) at every (q, k) of every shape, whatever the boxes"""
    kind, mode = launch
    ratio, what = _over_shapes(pc.check_floor, kind, mode, dev, name)
    extra = _pinned(kind, [pc.floor_interval(kind, *s) for s in pc.SHAPES])
    print("floor %s %s: worst error / bound %.3f at %s%s" % (_lid(launch), name, ratio, what, extra))
    assert ratio <= 1.0, (launch, ratio, what)


# ------------------------------------------------------------------------------------------------ 3. straddle set
@pytest.mark.parametrize("name", pc.SETS)
@pytest.mark.parametrize("launch", LAUNCHES, ids=_lid)
def test_straddle(dev, launch, name):
    """bg = 0, one-hot: the sign of one embedding entry decides the clamp"""
    kind, mode = launch
    ratio, what = _over_shapes(pc.check_straddle, kind, mode, dev, name)
    print("straddle %s %s: worst error / bound %.3f at %s" % (_lid(launch), name, ratio, what))
    assert ratio <= 1.0, (launch, ratio, what)


# ------------------------------------------------------------------------------------------------ 4. seeded weights
@pytest.mark.parametrize("name", pc.LATTICE_SETS)
@pytest.mark.parametrize("launch", LAUNCHES, ids=_lid)
def test_seeded_weights(dev, launch, name):
    """the seeded model's Wg on the lattice sets (self pairs included) within the per-pair bound"""
    kind, mode = launch
    ratio, what = _over_shapes(pc.check_seeded, kind, mode, dev, name)
    print("seeded %s %s: worst error / bound %.3f at %s" % (_lid(launch), name, ratio, what))
    assert ratio <= 1.0, (launch, ratio, what)


# ------------------------------------------------------------------------------------------------ 5. bit-equalities
@pytest.mark.parametrize("name", ["extremes", "wide1333", "self"])
def test_bit_equalities(dev, name):
    """tiled bf16 == mfma rows rounded to bf16 and batched == single (both 16-bit types), on the probe, straddle and floor
    weights over the extreme boxes: the stored values sit at both ends of the logit range (log 1e-6 ... log 100)"""
    weights = [pc.probe_weights(r, s, bias=b) for b in (pc.PROBE_BIAS, 0.0) for r, s in pc.PROBES] + [pc.floor_weights()]
    runners = {l: Runner(l[0], l[1], dev, name) for l in LAUNCHES if l[0] != "precise" and l[0] != "valu"}
    lo, hi = math.inf, -math.inf
    for wg_t, bg in weights:
        outs = {l: r.launch(wg_t, bg) for l, r in runners.items()}
        for shape in pc.SHAPES:
            rows = outs[("mfma", "single")][shape]
            one = outs[("tiled_bf16", "single")][shape]
            assert torch.equal(one, rows.to(torch.bfloat16).float()), (name, shape, "tiled bf16 != mfma rows rounded")
            assert torch.equal(outs[("tiled_bf16", "batched")][shape], one), (name, shape, "bf16 batched != single")
            assert torch.equal(outs[("tiled_f16", "batched")][shape], outs[("tiled_f16", "single")][shape]), (name, shape, "f16 batched != single")
            lo, hi = min(lo, float(rows.min())), max(hi, float(rows.max()))
    print("bit-equalities %s: %d weight sets x %d shapes, logits from %.4f to %.4f" % (name, len(weights), len(pc.SHAPES), lo, hi))
    assert lo < -13.8 and hi > 4.6
