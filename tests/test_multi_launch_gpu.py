"""-m gpu: the multi-problem launch forms of the kernels, called directly on ragged problems.

Every entry point here promises each problem the bits of its own single-problem call: the batched relation attention and
tile-ordered position logits (problems of different sizes, split counts and segment counts in one grid, chunked launches), the
ring / window-order / group forms of the FGFA aggregation (index tables that wrap, permute and share slots, NaN in the slots
no table names), flow_conv1_combine's three addressing modes and flow_pred_finish.  Bit-equality with the single calls, closeness
to float64 references of the same operands (tests/multi_launch_cases.py, checked on the CPU by test_multi_launch_twins.py),
and sentinel-filled guard bands round the outputs.
"""
import ctypes

import pytest
import torch

import cpu_ops
import multi_launch_cases as mc
from test_kernels_gpu import _relerr, _untile_pos

pytestmark = pytest.mark.gpu

HALF = (torch.bfloat16, torch.float16)
SENT16 = 0x7FFF          # a NaN in bf16 and in f16: no kernel here stores it


def _ops():
    from mega.pytorch_amd import ops
    return ops


def _lib():
    from mega.pytorch_amd import _lib as lib
    return lib


# ------------------------------------------------------------------------------------------------ 1. batched attention
def _attn_dev_item(it, dev, pos):
    d = {"q": it["q"].to(dev), "Nk": it["Nk"], "resid": it["resid"].to(dev), "bias_v": it["bias_v"].to(dev), "pos": pos}
    if it["N2"]:       # k2 / vt2 (and k / vt) as element-aligned views of wider buffers
        N1, N2, a, b = it["N1"], it["N2"], it["a_cols"], it["b_cols"]
        big1, big2, kb1, kb2 = (it[n].to(dev) for n in ("big1", "big2", "kb1", "kb2"))
        d.update(k=kb1[2:2 + N1], vt=big1[:, a:a + N1], N1=N1, k2=kb2[1:1 + N2], vt2=big2[:, b:b + N2])
    else:
        d.update(k=it["k"].to(dev), vt=it["vt"].to(dev))
    return d


def _attn_problems(shapes, dtype, dev, with_pos, resid_dtype=None):
    """-> (device items for ops.relation_attention_batched, float64 references)"""
    ops = _ops()
    wg, bg, dim_mat = (t.to(dev) for t in mc.attn_pos_weights())
    items, refs = [], []
    for i, shape in enumerate(shapes):
        it = mc.attn_item(shape, dtype, seed=i, resid_dtype=resid_dtype)
        pos = pos_ref = None
        if with_pos:       # f32 rows in f32 mode, tile-ordered 16-bit logits in the 16-bit modes
            half = dtype in HALF
            pos = ops.position_logits(it["rq"].to(dev), it["rk"].to(dev), wg, bg, dim_mat, precise=not half,
                                      tiled=dtype if half else False)
            pos_ref = _untile_pos(pos.cpu(), it["Nk"]) if half else pos.cpu()[:, :, :it["Nk"]]
        items.append(_attn_dev_item(it, dev, pos))
        refs.append(mc.relation_attention_f64(it["q"], it["k"], it["vt"], it["Nk"], pos=pos_ref, resid=it["resid"],
                                              bias_v=it["bias_v"]))
    return items, refs


@pytest.mark.parametrize("with_pos", [False, True], ids=["nopos", "pos"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_attention_batched_heterogeneous_problems(dev, dtype, with_pos):
    """Eight problems of different Nq (the grid's x extent is that of the largest: the others leave by the early exit),
    different split counts (two problems split their keys 3 ways, six do not: the z table and the combine kernel's skip) and
    one two-segment problem (the SEG build runs the seven one-segment problems) in ONE launch: every problem has the bits of
    its own single-problem launch, in either order of the list, and is close to the float64 formula on the same operands.
    The outputs are row blocks of one buffer -- problem i + 1 is the guard band of problem i -- so the single calls are made
    BEFORE the batched one.  16-bit modes: once more with f32 residuals (the io_f32 stream)."""
    ops = _ops()
    splits = [_lib().load().mega_relation_attention_splits(s[0], sum(s[1:]), 16) for s in mc.ATTN_ITEMS]
    assert _lib().load().mega_relation_attention_splits(40, 1500, 16) == 3
    assert splits == [1, 1, 1, 3, 1, 1, 3, 1]
    for resid_dtype in [None] + ([torch.float32] if dtype in HALF else []):
        items, refs = _attn_problems(mc.ATTN_ITEMS, dtype, dev, with_pos, resid_dtype)
        singles = [ops.relation_attention_batched([it])[0] for it in items]
        torch.cuda.synchronize()
        outs = ops.relation_attention_batched(items)
        back = ops.relation_attention_batched(items[::-1])[::-1]
        for i, shape in enumerate(mc.ATTN_ITEMS):
            what = (shape, dtype, with_pos, resid_dtype)
            assert outs[i].dtype == (resid_dtype or dtype) and tuple(outs[i].shape) == (shape[0], 1024)
            assert torch.isfinite(outs[i].float()).all(), what
            assert torch.equal(outs[i], singles[i]), (what, (outs[i].float() - singles[i].float()).abs().max().item())
            assert torch.equal(back[i], singles[i]), ("reversed list", what)
            err = _relerr(outs[i].cpu(), refs[i])
            print("attention batched %s: relerr %.3g" % (what, err))
            assert err < mc.ATTN_BOUND[dtype], (what, err)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_attention_batched_chunks_of_21(dev, dtype):
    """21 problems go out as two launches of 11 and 10 (at most 20 per launch, as even as possible)"""
    ops = _ops()
    assert ops._even_chunks(21, 20) == 11 and ops._MAX_BATCHED == 20
    items, refs = _attn_problems(mc.ATTN_CHUNK_ITEMS, dtype, dev, False)
    singles = [ops.relation_attention_batched([it])[0] for it in items]
    torch.cuda.synchronize()
    outs = ops.relation_attention_batched(items)
    assert len(outs) == 21
    for i, shape in enumerate(mc.ATTN_CHUNK_ITEMS):
        assert torch.isfinite(outs[i].float()).all() and torch.equal(outs[i], singles[i]), (i, shape, dtype)
        assert _relerr(outs[i].cpu(), refs[i]) < mc.ATTN_BOUND[dtype], (i, shape, dtype)


# ------------------------------------------------------------------------------------------------ 2. batched position logits
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_position_logits_batched_tiled(dev, dtype):
    """mega_position_logits_tiled_batched_dt: a grid sized by the largest Nq and Nk of the launch with a per-problem early
    exit.  Seven ragged problems in one launch and 23 in two (12 + 11): each has the bits of its single-problem call; three are
    also measured against the float64 formula on exp(), with the bounds of test_position_logits' fast-mode check (max 6e-3,
    mean 1e-3).  The 16-bit rounding of the stored logit stays inside them -- measured max 3.2e-3 / mean 3.6e-4 in bf16,
    4.4e-4 / 4.6e-5 in f16 -- so neither type gets a wider bound."""
    ops = _ops()
    wg_t, bg, dim_mat = mc.pos_weights()
    dargs = (wg_t.to(dev), bg.to(dev), dim_mat.to(dev))
    assert ops._even_chunks(23, 20) == 12
    for problems in (mc.POS_PROBLEMS, mc.POS_CHUNK_PROBLEMS):
        boxes = [mc.pos_problem(*p) for p in problems]
        qs, ks = [b[0].to(dev) for b in boxes], [b[1].to(dev) for b in boxes]
        singles = [ops.position_logits(q, k, *dargs, precise=False, tiled=dtype) for q, k in zip(qs, ks)]
        outs = ops.position_logits_batched(qs, ks, *dargs, precise=False, tiled=dtype)
        assert len(outs) == len(problems)
        for (Nq, Nk), (bq, bk), out, one in zip(problems, boxes, outs, singles):
            assert out.dtype == dtype and tuple(out.shape) == (16, (Nk + 31) // 32, Nq, 32)
            got = _untile_pos(out.cpu(), Nk)
            assert torch.isfinite(got).all() and torch.equal(got, _untile_pos(one.cpu(), Nk)), (Nq, Nk)
            if problems is mc.POS_PROBLEMS and (Nq, Nk) in mc.POS_F64_CHECKED:
                err = (got.double().exp() - mc.position_logits_f64(bq, bk, wg_t, bg).exp()).abs()
                print("position logits %s %s vs float64: max %.3g mean %.3g" % ((Nq, Nk), dtype, err.max(), err.mean()))
                assert err.max() < 6e-3 and err.mean() < 1e-3, ((Nq, Nk), err.max(), err.mean())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_position_logits_batched_guard_band(dev, dtype):
    """the seven-problem launch through the raw entry point, every output a 16-byte-aligned slice of ONE sentinel-filled
    buffer with 64 sentinel elements before, between and after: the sentinels survive, every slot of a key < Nk is written
    (pad-key slots of a last partial tile may hold anything) and holds the single-problem call's bits"""
    ops = _ops()
    lib = _lib().load()
    wg_t, bg, dim_mat = (t.to(dev) for t in mc.pos_weights())
    problems = mc.POS_PROBLEMS
    boxes = [mc.pos_problem(*p) for p in problems]
    qs, ks = [b[0].to(dev).contiguous() for b in boxes], [b[1].to(dev).contiguous() for b in boxes]
    singles = [ops.position_logits(q, k, wg_t, bg, dim_mat, precise=False, tiled=dtype).cpu() for q, k in zip(qs, ks)]
    gap = 64
    sizes = [16 * ((Nk + 31) // 32) * Nq * 32 for Nq, Nk in problems]
    offs, o = [], gap
    for n in sizes:
        offs.append(o)
        o += n + gap
    buf = torch.full((o,), SENT16, dtype=torch.int16, device=dev)
    arr = (ops._PosDesc * len(problems))()
    for i, (Nq, Nk) in enumerate(problems):
        assert (buf.data_ptr() + 2 * offs[i]) % 16 == 0
        arr[i].rois_q, arr[i].rois_k, arr[i].out = qs[i].data_ptr(), ks[i].data_ptr(), buf.data_ptr() + 2 * offs[i]
        arr[i].Nq, arr[i].Nk = Nq, Nk
    rc = lib.mega_position_logits_tiled_batched_dt(ctypes.addressof(arr), len(problems), wg_t.data_ptr(), bg.data_ptr(),
                                                   dim_mat.data_ptr(), ops._DT[dtype], ops._stream())
    _lib().check(rc, "mega_position_logits_tiled_batched_dt")
    torch.cuda.synchronize()
    host = buf.cpu()
    end = 0
    for (Nq, Nk), off, n, one in zip(problems, offs, sizes, singles):
        assert (host[end:off] == SENT16).all(), "sentinel before problem %s overwritten" % ((Nq, Nk),)
        sl = host[off:off + n].view(16, (Nk + 31) // 32, Nq, 32)
        # (_untile_pos on the raw 16-bit integers: the slots of the keys < Nk, as exact floats)
        assert (_untile_pos(sl, Nk) != float(SENT16)).all(), "problem %s: a slot of a key < Nk was not written" % ((Nq, Nk),)
        assert torch.equal(_untile_pos(sl.view(dtype), Nk), _untile_pos(one, Nk)), (Nq, Nk)
        end = off + n
    assert (host[end:] == SENT16).all() and host.numel() - end == gap


# ------------------------------------------------------------------------------------------------ 2b. single C entry points
def _single_attention(lib, ptrs, ldv, Nq, Nk, dtype, pos, ldp, out, ws, ws_bytes, tiled=False):
    """mega_relation_attention (no position term, or f32 rows `pos` with ldp) or, tiled, mega_relation_attention_tiled_pos_dt on
    ptrs = the addresses of (q, k, vt, resid, bias_v) -> the return code"""
    ops = _ops()
    q, k, vt, resid, bias_v = ptrs
    head = (q, 1024, k, 1024, vt, ldv)
    tail = (resid, 1024, bias_v, out, 1024, Nq, Nk, 16, 0.125, ops._DT[dtype], ws, ws_bytes, ops._stream())
    if tiled:
        return lib.mega_relation_attention_tiled_pos_dt(*head, pos, *tail)
    return lib.mega_relation_attention(*head, pos, ldp, *tail)


def test_single_entry_points_are_batches_of_one(dev):
    """mega_position_logits_tiled_dt, mega_relation_attention_tiled_pos_dt and mega_relation_attention, which no Python wrapper
    calls any more (ops.relation_attention and the tiled ops.position_logits are one-problem calls of the batched wrappers):
    each fills one descriptor and goes through the batched launcher, so its output has the bits of the one-problem
    ops.*_batched call on the same operands and is within the batched tests' bounds of the float64 formula.
      bf16 35 x 97: the tile-ordered logits, then the attention on them with a bf16 residual.  The boxes are
        mc.pos_problem's: the exact f32 formula is itself 2.8e-4 (max) / 4.3e-7 (mean) from float64 on exp() there, well
        inside the 6e-3 / 1e-3 the fast kernel is allowed;
      f32 3 x 33: f32 `pos` rows with ldp = 64 from mega_position_logits(precise=1);
      bf16 40 x 1500, no position term: with its workspace (3 key-range splits: the combine launch) and with ws = NULL
        (unsplit: another summation order, so measured against the float64 formula only).
    Nq = 0 returns MEGA_OK before any pointer check; a NULL q with Nq > 0 is MEGA_ERR_ARG."""
    ops = _ops()
    lib = _lib().load()

    def item(shape, dtype, seed):
        it = mc.attn_item(shape, dtype, seed=seed)
        it["dev"] = tuple(it[n].to(dev) for n in ("q", "k", "vt", "resid", "bias_v"))
        it["ptrs"] = tuple(t.data_ptr() for t in it["dev"])
        return it

    def single(it, pos, ldp, out, ws=None, ws_bytes=0, tiled=False):
        return _single_attention(lib, it["ptrs"], it["vt"].shape[1], it["Nq"], it["Nk"], it["q"].dtype, pos, ldp,
                                 out.data_ptr(), ws, ws_bytes, tiled)

    def batched_of_one(it, pos):
        q, k, vt, resid, bias_v = it["dev"]
        return ops.relation_attention_batched([{"q": q, "k": k, "vt": vt, "Nk": it["Nk"], "pos": pos, "resid": resid,
                                                "bias_v": bias_v}])[0]

    def check(what, out, it, pos_ref, want=None):
        dtype = it["q"].dtype
        ref = mc.relation_attention_f64(it["q"], it["k"], it["vt"], it["Nk"], pos=pos_ref, resid=it["resid"], bias_v=it["bias_v"])
        err = _relerr(out.cpu(), ref)
        print("single entry %s: relerr %.3g" % (what, err))
        assert torch.isfinite(out.float()).all() and err < mc.ATTN_BOUND[dtype], (what, err)
        if want is not None:
            assert torch.equal(out, want), (what, (out.float() - want.float()).abs().max().item())

    # ---- bf16 35 x 97: tile-ordered logits, then the attention that reads them
    dt = torch.bfloat16
    Nq, Nk = 35, 97
    it = item((Nq, Nk), dt, 1)
    wg_t, bg, dim_mat = mc.pos_weights()
    bq, bk = mc.pos_problem(Nq, Nk)
    dargs = (wg_t.to(dev), bg.to(dev), dim_mat.to(dev))
    bq_d, bk_d = bq.to(dev).contiguous(), bk.to(dev).contiguous()
    pos = torch.full((16, (Nk + 31) // 32, Nq, 32), SENT16, dtype=torch.int16, device=dev).view(dt)
    rc = lib.mega_position_logits_tiled_dt(bq_d.data_ptr(), bk_d.data_ptr(), *(t.data_ptr() for t in dargs), pos.data_ptr(),
                                           Nq, Nk, ops._DT[dt], ops._stream())
    assert rc == 0
    pos_b = ops.position_logits_batched([bq_d], [bk_d], *dargs, precise=False, tiled=dt)[0]
    got = _untile_pos(pos.cpu(), Nk)
    assert torch.isfinite(got).all() and torch.equal(got, _untile_pos(pos_b.cpu(), Nk))
    err = (got.double().exp() - mc.position_logits_f64(bq, bk, wg_t, bg).exp()).abs()
    print("single entry position logits (%d, %d) vs float64: max %.3g mean %.3g" % (Nq, Nk, err.max(), err.mean()))
    assert err.max() < 6e-3 and err.mean() < 1e-3, (err.max(), err.mean())
    out = torch.empty((Nq, 1024), dtype=dt, device=dev)
    assert lib.mega_relation_attention_splits(Nq, Nk, 16) == 1
    assert single(it, pos.data_ptr(), 0, out, tiled=True) == 0
    check("tiled_pos_dt bf16 (35, 97)", out, it, got, want=batched_of_one(it, pos_b))

    # ---- f32 3 x 33: f32 position rows with a leading dimension
    Nq, Nk = 3, 33
    it = item((Nq, Nk), torch.float32, 2)
    wg, bg2, dm2 = (t.to(dev) for t in mc.attn_pos_weights())
    rows = torch.empty((16, Nq, 64), dtype=torch.float32, device=dev)
    rc = lib.mega_position_logits(it["rq"].to(dev).data_ptr(), it["rk"].to(dev).data_ptr(), wg.data_ptr(), bg2.data_ptr(),
                                  dm2.data_ptr(), rows.data_ptr(), Nq, Nk, 64, 1, ops._stream())
    assert rc == 0
    out = torch.empty((Nq, 1024), dtype=torch.float32, device=dev)
    assert single(it, rows.data_ptr(), 64, out) == 0
    check("f32 (3, 33) pos rows", out, it, rows.cpu()[:, :, :Nk], want=batched_of_one(it, rows))

    # ---- bf16 40 x 1500, no position term: split 3 ways with the workspace, unsplit without
    Nq, Nk = 40, 1500
    it = item((Nq, Nk), dt, 3)
    assert lib.mega_relation_attention_splits(Nq, Nk, 16) == 3
    nb = lib.mega_relation_attention_workspace_bytes(Nq, Nk, 16)
    assert nb > 0
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    want = batched_of_one(it, None)
    out = torch.empty((Nq, 1024), dtype=dt, device=dev)
    assert single(it, None, 0, out, ws.data_ptr(), nb) == 0
    check("bf16 (40, 1500) three splits", out, it, None, want=want)
    out1 = torch.empty((Nq, 1024), dtype=dt, device=dev)
    assert single(it, None, 0, out1) == 0
    check("bf16 (40, 1500) ws = NULL", out1, it, None)

    # ---- the contract's early returns
    nulls = (None,) * 5                            # every pointer NULL: Nq = 0 returns before looking at any
    for tiled in (False, True):
        assert _single_attention(lib, nulls, 0, 0, Nk, dt, None, 0, None, None, 0, tiled) == 0
        assert _single_attention(lib, (None,) + it["ptrs"][1:], it["vt"].shape[1], Nq, Nk, dt, None, 0, out.data_ptr(), None, 0,
                                 tiled) == 1       # q = NULL with Nq = 40
    assert lib.mega_position_logits_tiled_dt(None, None, None, None, None, None, 0, 97, ops._DT[dt], ops._stream()) == 0
    assert lib.mega_position_logits_tiled_dt(None, bk_d.data_ptr(), *(t.data_ptr() for t in dargs), pos.data_ptr(), 35, 97,
                                             ops._DT[dt], ops._stream()) == 1
    torch.cuda.synchronize()
    assert torch.equal(out, want)                  # (the refused calls launched nothing)


# ------------------------------------------------------------------------------------------------ 3. FGFA ring / window / group
FGFA_W_BOUND = {torch.float32: 2e-5, torch.bfloat16: 2e-3}        # test_fgfa_warp_aggregate's bounds
FGFA_O_BOUND = {torch.float32: 1e-5, torch.bfloat16: 1e-2}


def _padded(shape, dtype, dev, pad=64, fill=-7.0):
    """-> (flat sentinel-filled buffer, contiguous view of `shape` in its middle, check(): the sentinels are intact)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    view = buf[pad:pad + n].view(*shape)

    def intact():
        h = buf.cpu()
        return bool((h[:pad] == fill).all() and (h[pad + n:] == fill).all())
    return buf, view, intact


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geometry", mc.FGFA_GEOMETRIES)
def test_fgfa_ring_and_window_order_forms(dev, geometry, dtype):
    """mega_fgfa_warp_aggregate_ring / _ring_pos: the window's T maps live in a ring of S slots, named by a table
    [key slot, slot of window position 0 .. T-1] -- a window that wraps round the ring and a shuffled one, the key frame at
    window position 0, T - 1 and T // 2, NaN in every slot (features and flow) the table does not name.  A table row is
    [slots[key_pos]] + slots: the window-order form reads the key frame's features from order[0] and its flow field from
    window position key_pos, so its contract is order[0] == order[1 + key_pos].  Outputs AND weights have the bits of the
    contiguous call on the re-ordered frames; the ring form is also measured against the oracle in float64, and writes
    through out= into the middle of a sentinel-filled buffer."""
    ops = _ops()
    S, T, H, W, Cf, Ce = geometry
    ring0, flow0 = mc.fgfa_ring(geometry, dtype)
    for slots in (mc.wrapped_slots(S, T), mc.shuffled_slots(S, T, seed=S + T)):
        ring, flow_by_slot = mc.nan_unused(ring0, slots), mc.nan_unused(flow0, slots)
        assert (S == T) or not torch.isfinite(ring.float()).all()
        idx = torch.tensor(slots)
        ring_d, flow_d = ring.to(dev), flow_by_slot.to(dev)
        cont_feats, cont_flow = ring[idx].contiguous().to(dev), flow_by_slot[idx].contiguous().to(dev)
        for key_pos in (0, T - 1, T // 2):
            row = mc.order_row(slots, key_pos)
            assert row[0] == row[1 + key_pos]
            order = mc.orders_tensor(row).to(dev)
            want, want_w = ops.fgfa_warp_aggregate(cont_feats, cont_flow, Cf, key_pos, want_weights=True)
            _, view, intact = _padded((H, W, Cf), dtype, dev)
            a, aw = ops.fgfa_warp_aggregate(ring_d, flow_d, Cf, 0, want_weights=True, order=order, out=view)
            b, bw = ops.fgfa_warp_aggregate(ring_d, cont_flow, Cf, 0, want_weights=True, order=order, flow_pos=key_pos)
            what = (geometry, dtype, slots, key_pos)
            assert a.data_ptr() == view.data_ptr() and intact(), what
            assert torch.isfinite(a.float()).all() and torch.isfinite(aw).all(), what
            assert torch.equal(a, want) and torch.equal(aw, want_w), ("ring form", what)
            assert torch.equal(b, want) and torch.equal(bw, want_w), ("window-order form", what)
            ref, ref_w = mc.fgfa_aggregate_f64(ring, flow_by_slot[idx], slots, key_pos, Cf)
            werr, err = (aw.cpu().double() - ref_w).abs().max().item(), _relerr(a.cpu(), ref)
            print("fgfa ring %s: weights %.3g out %.3g" % (what, werr, err))
            assert werr < FGFA_W_BOUND[dtype] and err < FGFA_O_BOUND[dtype], (what, werr, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geometry", mc.FGFA_GEOMETRIES)
def test_fgfa_group_form(dev, geometry, dtype):
    """mega_fgfa_warp_aggregate_ring_pos_batched: G key frames in one grid, each with its own table row (neighbouring windows
    share T - 1 slots; some rows are shuffled), its own T flow fields and its own output map.  G = 1 too: the kernel applies
    its per-key-frame offsets only when gridDim.y > 1.  Each map has the bits of its own window-order call; the raw entry
    point with weights_out (no wrapper passes it: the [G][T][H][W] offset) gives each key frame the single call's weights,
    inside sentinel-padded output and weight buffers."""
    ops = _ops()
    lib = _lib().load()
    S, T, H, W, Cf, Ce = geometry
    ring0, _ = mc.fgfa_ring(geometry, dtype)
    for G in (1, 2, 5):
        rows = mc.group_slots(S, T, G)
        assert len({tuple(r) for r in rows}) == G and (G == 1 or set(rows[0]) & set(rows[1]))
        ring = mc.nan_unused(ring0, {s for r in rows for s in r}).to(dev)
        flows = mc.fgfa_flow(torch.Generator().manual_seed(G), G * T, H, W).to(dev)
        for key_pos in (0, T - 1, T // 2):
            orders = mc.orders_tensor([mc.order_row(r, key_pos) for r in rows]).to(dev)
            singles = [ops.fgfa_warp_aggregate(ring, flows[g * T:(g + 1) * T], Cf, 0, want_weights=True, order=orders[g],
                                               flow_pos=key_pos) for g in range(G)]
            got = ops.fgfa_warp_aggregate_group(ring, flows, Cf, orders, key_pos)
            assert tuple(got.shape) == (G, H, W, Cf) and torch.isfinite(got.float()).all()
            for g in range(G):
                assert torch.equal(got[g], singles[g][0]), (geometry, dtype, G, key_pos, g)
            if key_pos != T // 2:
                continue
            _, out, out_intact = _padded((G, H, W, Cf), dtype, dev)
            _, wts, wts_intact = _padded((G, T, H, W), torch.float32, dev)
            rc = lib.mega_fgfa_warp_aggregate_ring_pos_batched(ring.data_ptr(), flows.data_ptr(), out.data_ptr(), wts.data_ptr(),
                                                               T, H, W, Cf, Ce, orders.data_ptr(), key_pos, G, ops._dt(ring),
                                                               ops._stream())
            _lib().check(rc, "mega_fgfa_warp_aggregate_ring_pos_batched")
            torch.cuda.synchronize()
            assert out_intact() and wts_intact(), (geometry, dtype, G)
            for g in range(G):
                assert torch.equal(out[g], singles[g][0]) and torch.equal(wts[g], singles[g][1]), (geometry, dtype, G, g)


# ------------------------------------------------------------------------------------------------ 4. FlowNetS pieces
def _conv1_check(dev, ab, bias, dtype, T_out, order=None, **kw):
    """ops.flow_conv1_combine == the twin, bit for bit, as a fresh tensor and through out= inside a sentinel buffer"""
    ops = _ops()
    h, w = ab.shape[1:3]
    want = cpu_ops.flow_conv1_combine(ab, bias, dtype, order=order, **kw)
    assert tuple(want.shape) == (T_out, h, w, 64) and torch.isfinite(want.float()).all()
    order_d = None if order is None else order.to(dev)
    got = ops.flow_conv1_combine(ab.to(dev), bias.to(dev), dtype, order=order_d, **kw)
    assert got.dtype == dtype and torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), kw
    n = T_out * h * w * 64
    buf = torch.full((n + 128,), SENT16, dtype=torch.int16, device=dev)
    out = buf[64:64 + n].view(dtype).view(T_out, h, w, 64)
    ops.flow_conv1_combine(ab.to(dev), bias.to(dev), dtype, order=order_d, out=out, **kw)
    host = buf.cpu()
    assert (host[:64] == SENT16).all() and (host[64 + n:] == SENT16).all(), kw
    assert torch.equal(host[64:64 + n].view(T_out, h, w, 64), want.view(torch.int16)), kw


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", mc.CONV1_SHAPES)
def test_flow_conv1_combine_three_modes(dev, shape, dtype):
    """leaky(A[key slot] + B[slot] + bias) from ab = [A | B] per ring slot, NaN in the slots no pair names.  The twin's
    arithmetic is the kernel's (an f32 add of A, B and the bias in that order, * 0.1 for the negatives -- no FMA can form --
    then one rounding to the 16-bit type), so the comparison is on the bits."""
    S, h, w = shape
    ab0, bias = mc.conv1_inputs(S, h, w)
    # key = k: the pairs (slot k, slot t) for t < T, with T < S
    T = S - 2
    _conv1_check(dev, mc.nan_unused(ab0, range(T)), bias, dtype, T, key=T // 2, T=T)
    # order (1-D): the key frame's slot is order[0]; T = S, every slot in use
    _conv1_check(dev, ab0, bias, dtype, S, order=mc.orders_tensor([S - 1] + list(range(S))))
    # nwin > 0: [G, 1 + nwin] tables, wrapped and permuted windows, key slots outside their own window
    nwin = S - 2
    for G in (1, 3):
        rows = mc.conv1_group_orders(S, G, nwin)
        assert all(r[0] not in r[1:] for r in rows)
        ab = mc.nan_unused(ab0, {s for r in rows for s in r})
        _conv1_check(dev, ab, bias, dtype, G * nwin, order=mc.orders_tensor(rows), nwin=nwin)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_flow_conv1_combine_grid_stride_loop(dev, dtype):
    """more work items (T P 8 = 8.6 M) than the 32768 x 256 threads of the capped grid: the first 212 992 threads run the
    loop twice, for the second half of the LAST pair's pixels.  G = 3 key frames x 7 window positions on a ring of 4 slots,
    P = 64 x 800; every 97th pixel, the first and the last 64 pixels of every pair are compared with the twin."""
    ops = _ops()
    S, G, nwin, h, w = 4, 3, 7, 64, 800
    P, T = h * w, G * nwin
    assert T * P * 8 > 32768 * 256
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    ab = torch.randn((S, h, w, 128), generator=g, device=dev)
    bias = torch.randn((64,), generator=g, device=dev) * 0.5
    rows = [[gi] + [(gi + 1 + 3 * t) % S for t in range(nwin)] for gi in range(G)]
    got = ops.flow_conv1_combine(ab, bias, dtype, order=mc.orders_tensor(rows).to(dev), nwin=nwin)
    assert tuple(got.shape) == (T, h, w, 64)
    ps = torch.tensor(sorted(set(range(0, P, 97)) | set(range(P - 64, P))))
    assert int(ps[0]) == 0 and int(ps[-1]) == P - 1 and (T - 1) * P + int(ps[-1]) >= 32768 * 256 // 8
    sub = ab.view(S, P, 128)[:, ps.to(dev)].cpu().view(S, 1, ps.numel(), 128)
    want = cpu_ops.flow_conv1_combine(sub, bias.cpu(), dtype, order=mc.orders_tensor(rows), nwin=nwin)
    got_s = got.view(T, P, 64)[:, ps.to(dev)].cpu()
    assert torch.equal(got_s.view(torch.int16), want.view(T, ps.numel(), 64).view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", mc.PRED_SHAPES)
def test_flow_pred_finish_borders_and_image_seams(dev, shape, dtype):
    """(sum of the nine shifted taps, zero padding) * scale + bias against the same in float64.  The bound is the kernel's
    own round-off: nine f32 additions and one fused multiply-add, each within 2^-24 of its result's size -- together under
    10 * 2^-24 * (sum of |taps| * |scale| + |bias|) -- plus the one rounding to the output type, half an ulp at |ref|
    (2^-24 / 2^-8 / 2^-11 of the binade for f32 / bf16 / f16: bf16 has 8 significant bits, so a correctly rounded bf16 result
    is up to 2^-8, not 2^-9, of its binade away; measured worst error / bound: 0.20 in f32, 0.996 in bf16 and f16, i.e. the
    16-bit outputs are correctly rounded and the bound has no slack).  Borders and the seam between
    images are the point: image n + 1 is 16 x image n, so a row of the wrong image in a sum is far outside the bound; the
    columns 18 .. ldz-1 of z hold NaN and must not be read."""
    ops = _ops()
    N, H, W, ldz = shape
    z, bias = mc.pred_inputs(N, H, W, ldz)
    for scale in (1.0, 2.5):
        got = ops.flow_pred_finish(z.to(dev), bias.to(dev), scale, dtype).cpu()
        assert got.dtype == dtype and tuple(got.shape) == (N, H, W, 2) and torch.isfinite(got.float()).all()
        ref, mag = mc.flow_pred_finish_f64(z, bias, scale)
        bound = 10 * 2.0 ** -24 * mag + mc.half_ulp(ref, dtype)
        err = (got.double() - ref).abs()
        print("flow_pred_finish %s %s scale %.1f: worst error / bound %.3f" % (shape, dtype, scale, (err / bound).max()))
        assert (err <= bound).all(), (shape, dtype, scale, (err / bound).max().item())
