"""-m gpu: the 16-bit relation attention (and the tile-ordered position logits it consumes) against bits RECORDED from
the kernel as it stood before its scheduling was first changed (dead query waves skip the tile arithmetic; later: other
staging of the K / V^T tiles).  Such changes move no arithmetic, so every output must stay bit-identical.

tests/golden/attention_bits.npz holds, per case, the SHA-256 of the output's bytes and a small strided sample of its bit
pattern (the sample only says where a mismatch lies).  The inputs are regenerated here from numpy's legacy seeded
generator (a frozen stream).  Recorded with `python tests/test_attention_ring_gpu.py --record` on an MI355X.

So that a bad recording cannot pass silently, every output is also checked to be finite and to agree with the CPU twin
(tests/cpu_ops.py) within the bound tests/test_kernels_gpu.py uses for the attention's hot shapes.

Geometry (Nq x Nk, N1 = first key of the second segment or None):
  Nq 3 (one live wave), 35 (a partial wave + dead waves), 129 (a second block with one row), 300 (2 of 12 waves dead);
  Nk 31, 32, 33, 96, 97, 128, 129: fewer 32-key tiles than a 3- or 4-deep tile ring, exactly the ring, a wrap, odd counts;
  N1 32, 64, 75, Nk - 1: seam at a tile boundary, mid-tile (75, and a V^T second segment that starts at a 2-byte-aligned
  column), one-key second segment; the N1 = 64 problems hand over a 16-byte-aligned second V^T segment, the others not;
  one launch mixing three problems of different (Nq, Nk, N1): blocks past a problem's Nq and dead waves in one grid;
  one problem small enough to split its key range (40 x 1500: 3 splits + the combine kernel), with and without a seam.
Each for bf16 and f16, with and without the tiled position term, with the f32 residual stream (io_f32) on and off.
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bits.npz")
NQS = (3, 35, 129, 300)
NKS = (31, 32, 33, 96, 97, 128, 129)
BOUND = {"bfloat16": 3e-2, "float16": 4e-3}          # test_relation_attention_hot_shapes' bounds
COMBOS = [(d, p, f) for d in ("bfloat16", "float16") for p in (False, True) for f in (False, True)]


def _n1_choices(Nk):
    return [n for n in (None, 32, 64, 75, Nk - 1) if n is None or 0 < n < Nk]


def _geometries():
    """every (Nq, Nk) pair; N1 walks through its choices so that each value meets each Nq and most Nk"""
    out, j = [], 0
    for Nk in NKS:
        ch = _n1_choices(Nk)
        for Nq in NQS:
            out.append((Nq, Nk, ch[j % len(ch)]))
            j += 1
    # seams the walk above does not reach at the 2-of-12 dead-wave shape and at the wraps
    out += [(300, 129, 75), (300, 128, 64), (300, 97, 96), (300, 96, 32), (35, 129, 75), (129, 97, 75)]
    return list(dict.fromkeys(out))


MIXED = [(300, 129, 75), (35, 33, None), (129, 97, 64)]
SPLIT = [(40, 1500, None), (40, 1500, 75)]


def _randn(rs, shape, scale=1.0, shift=0.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale + shift).astype(np.float32))


def _problem(seed, Nq, Nk, N1, dt, with_pos, io_f32, dev, ops):
    """-> (item for ops.relation_attention_batched, the same problem for the CPU twin, the tiled logits or None)"""
    rs = np.random.RandomState(seed)
    q = _randn(rs, (Nq, 1024), 0.3).to(dt)
    kfull = _randn(rs, (Nk, 1024), 0.3).to(dt)
    vfull = _randn(rs, (1024, Nk), 1.0, 0.5).to(dt)
    resid = _randn(rs, (Nq, 1024))
    resid = resid if io_f32 else resid.to(dt)
    bv = _randn(rs, (1024,), 0.1)
    pos = pos_rows = None
    if with_pos:
        rq = torch.from_numpy(rs.uniform(0, 100, (Nq, 4)).astype(np.float32))
        rq[:, 2:] += rq[:, :2] + 5
        rk = torch.from_numpy(rs.uniform(0, 100, (Nk, 4)).astype(np.float32))
        rk[:, 2:] += rk[:, :2] + 5
        wg = _randn(rs, (64, 16), 0.3)
        bg = _randn(rs, (16,), 0.1, 0.3)
        dim_mat = torch.full((8,), 1000.0).pow(torch.arange(8) / 8.0)
        pos = ops.position_logits(rq.to(dev), rk.to(dev), wg.to(dev), bg.to(dev), dim_mat.to(dev), precise=False, tiled=dt)
        G, KT = 16, (Nk + 31) // 32
        x = pos.float().cpu().view(G, KT, Nq, 2, 4, 4).permute(0, 2, 1, 4, 3, 5)     # key = 8 rq + 4 h2 + e
        pos_rows = x.reshape(G, Nq, KT * 32)
    ld = (Nk + 31) // 32 * 32
    vt = torch.zeros((1024, ld), dtype=dt)
    vt[:, :Nk] = vfull
    twin = {"q": q, "k": kfull, "vt": vt, "Nk": Nk, "resid": resid, "bias_v": bv, "pos": pos_rows}
    item = {"q": q.to(dev), "Nk": Nk, "resid": resid.to(dev), "bias_v": bv.to(dev), "pos": pos}
    if N1 is None:
        item.update(k=kfull.to(dev), vt=vt.to(dev))
        return item, twin, pos
    # two segments inside wider buffers: K rows after other rows, V^T column blocks.  The second V^T block starts
    # 16-byte aligned with a 16-byte row pitch when N1 == 64, at an odd element (2-byte alignment) otherwise.
    N2 = Nk - N1
    b_cols, w2 = (8, (8 + N2 + 15) // 8 * 8) if N1 == 64 else (5, 5 + N2 + 11)
    big1 = torch.full((1024, (8 + N1 + 16) // 8 * 8), 7.0, dtype=dt)
    big1[:, 8:8 + N1] = vfull[:, :N1]
    big2 = torch.full((1024, w2), -3.0, dtype=dt)
    big2[:, b_cols:b_cols + N2] = vfull[:, N1:]
    kb1 = torch.zeros((2 + N1 + 1, 1024), dtype=dt)
    kb1[2:2 + N1] = kfull[:N1]
    kb2 = torch.zeros((1 + N2 + 3, 1024), dtype=dt)
    kb2[1:1 + N2] = kfull[N1:]
    big1, big2, kb1, kb2 = big1.to(dev), big2.to(dev), kb1.to(dev), kb2.to(dev)
    item.update(k=kb1[2:2 + N1], vt=big1[:, 8:8 + N1], N1=N1, k2=kb2[1:1 + N2], vt2=big2[:, b_cols:b_cols + N2])
    if N1 == 64:
        assert item["vt2"].data_ptr() % 16 == 0 and (big2.stride(0) * big2.element_size()) % 16 == 0
    else:
        assert item["vt2"].data_ptr() % 16 != 0
    return item, twin, pos


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def _record(name, t, got):
    b = _bits(t)
    got[name + "/sha"] = np.frombuffer(hashlib.sha256(b.tobytes()).digest(), dtype=np.uint8)
    b2 = b.reshape(-1, b.shape[-1])
    got[name + "/sample"] = b2[::max(1, b2.shape[0] // 8), ::64].copy()


def run_combo(dev, dtype, with_pos, io_f32):
    """Runs every case of one (dtype, position term, io_f32) combination.  -> ({name: bits record}, [(name, out, twin)])"""
    from mega.pytorch_amd import ops
    dt = getattr(torch, dtype)
    tag = "%s/pos%d/f32io%d" % (dtype, with_pos, io_f32)
    got, checks = {}, []

    def launch(names_geoms):
        items, twins = [], []
        for name, (Nq, Nk, N1) in names_geoms:
            seed = (Nq * 7919 + Nk * 31 + (N1 or 0)) % (2 ** 31)
            item, twin, pos = _problem(seed, Nq, Nk, N1, dt, with_pos, io_f32, dev, ops)
            items.append(item)
            twins.append(twin)
            if pos is not None:
                _record("%s/%s/pos" % (tag, name), pos, got)
        outs = ops.relation_attention_batched(items)
        torch.cuda.synchronize()
        for (name, _), out, twin in zip(names_geoms, outs, twins):
            assert out.dtype == (torch.float32 if io_f32 else dt)
            _record("%s/%s/out" % (tag, name), out, got)
            checks.append(("%s/%s" % (tag, name), out.float().cpu(), twin))

    for geom in _geometries():
        launch([("one_%d_%d_%s" % geom, geom)])
    launch([("mixed%d_%d_%d_%s" % ((i,) + geom), geom) for i, geom in enumerate(MIXED)])
    for geom in SPLIT:
        assert ops._lib.load().mega_relation_attention_splits(geom[0], geom[1], 16) > 1
        launch([("split_%d_%d_%s" % geom, geom)])
    return got, checks


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("dtype,with_pos,io_f32", COMBOS)
def test_attention_bits_unchanged(dev, golden, dtype, with_pos, io_f32):
    import cpu_ops
    got, checks = run_combo(dev, dtype, with_pos, io_f32)
    # (i) sane on its own: finite, and the CPU twin's result within the hot-shape bound
    for name, out, tw in checks:
        assert torch.isfinite(out).all(), name
        ref = cpu_ops.relation_attention(tw["q"], tw["k"], tw["vt"], tw["Nk"], pos=tw["pos"], resid=tw["resid"],
                                         bias_v=tw["bias_v"]).float()
        err = ((out.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-12)).item()
        assert err < BOUND[dtype], "%s: relerr %.3g against the CPU twin" % (name, err)
    # (ii) the recorded bits
    bad = []
    for key, val in got.items():
        assert key in golden, "no recording for %s" % key
        if key.endswith("/sha") and not np.array_equal(val, golden[key]):
            s = key[:-4] + "/sample"
            bad.append("%s (%d of %d sampled elements differ)" % (key[:-4], int((got[s] != golden[s]).sum()), got[s].size))
    assert not bad, "%d outputs differ from the recorded bits: %s" % (len(bad), "; ".join(bad[:8]))


def test_recording_covers_exactly_these_cases(golden):
    """the fixture holds a record for every case above and nothing else (no GPU work: names only)"""
    want = set()
    for dtype, with_pos, io_f32 in COMBOS:
        tag = "%s/pos%d/f32io%d" % (dtype, with_pos, io_f32)
        names = ["one_%d_%d_%s" % g for g in _geometries()] + ["mixed%d_%d_%d_%s" % ((i,) + g) for i, g in enumerate(MIXED)] + \
            ["split_%d_%d_%s" % g for g in SPLIT]
        for n in names:
            for what in (("out", "pos") if with_pos else ("out",)):
                want.update({"%s/%s/%s/sha" % (tag, n, what), "%s/%s/%s/sample" % (tag, n, what)})
    assert set(golden.keys()) == want


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rec = {}
    for c in COMBOS:
        rec.update(run_combo(torch.device("cuda:0"), *c)[0])
    dst = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN
    np.savez_compressed(dst, **rec)
    print("recorded %d arrays -> %s (%d bytes)" % (len(rec), dst, os.path.getsize(dst)))
