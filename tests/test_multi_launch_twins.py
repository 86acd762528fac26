"""The references of tests/test_multi_launch_gpu.py checked against each other on the CPU, so that a wrong twin cannot hide a
wrong kernel: the ring / window-order / group forms of the twins against their contiguous and single-call forms, the float64
restatements against the f32 twins, and flow_pred_finish against the 3 x 3 convolution it is one half of."""
import pytest
import torch
import torch.nn.functional as F

import cpu_ops
import multi_launch_cases as mc


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geometry", mc.FGFA_GEOMETRIES + [(7, 5, 4, 6, 8, 8)])
def test_fgfa_twin_ring_and_window_order_equal_contiguous(geometry, dtype):
    S, T, H, W, Cf, Ce = geometry
    ring0, flow0 = mc.fgfa_ring(geometry, dtype)
    for slots in (mc.wrapped_slots(S, T), mc.shuffled_slots(S, T, seed=S + T)):
        ring, flow_by_slot = mc.nan_unused(ring0, slots), mc.nan_unused(flow0, slots)
        idx = torch.tensor(slots)
        for key_pos in (0, T - 1, T // 2):
            order = mc.orders_tensor(mc.order_row(slots, key_pos))
            assert int(order[0]) == int(order[1 + key_pos])
            want, want_w = cpu_ops.fgfa_warp_aggregate(ring[idx], flow_by_slot[idx], Cf, key_pos, want_weights=True)
            a, aw = cpu_ops.fgfa_warp_aggregate(ring, flow_by_slot, Cf, 0, want_weights=True, order=order)
            b, bw = cpu_ops.fgfa_warp_aggregate(ring, flow_by_slot[idx], Cf, 0, want_weights=True, order=order,
                                                flow_pos=key_pos)
            assert torch.isfinite(want.float()).all() and torch.isfinite(want_w).all()
            assert torch.equal(a, want) and torch.equal(aw, want_w)
            assert torch.equal(b, want) and torch.equal(bw, want_w)
            # the float64 restatement the GPU test measures against
            ref, ref_w = mc.fgfa_aggregate_f64(ring, flow_by_slot[idx], slots, key_pos, Cf)
            assert (want_w.double() - ref_w).abs().max() < 2e-5
            err = ((want.double() - ref).abs().max() / ref.abs().max()).item()
            assert err < (1e-5 if dtype == torch.float32 else 2.0 ** -8), err    # (bf16: the twin's one output rounding)


@pytest.mark.parametrize("G", [1, 2, 5])
def test_fgfa_twin_group_equals_stack_of_single_calls(G):
    geometry = mc.FGFA_GEOMETRIES[0]
    S, T, H, W, Cf, Ce = geometry
    ring0, _ = mc.fgfa_ring(geometry, torch.float32)
    rows = mc.group_slots(S, T, G)
    assert len({tuple(r) for r in rows}) == G
    ring = mc.nan_unused(ring0, {s for r in rows for s in r})
    flows = mc.fgfa_flow(torch.Generator().manual_seed(G), G * T, H, W)
    for key_pos in (0, T - 1, T // 2):
        orders = mc.orders_tensor([mc.order_row(r, key_pos) for r in rows])
        got = cpu_ops.fgfa_warp_aggregate_group(ring, flows, Cf, orders, key_pos)
        assert tuple(got.shape) == (G, H, W, Cf) and torch.isfinite(got).all()
        for gi in range(G):
            idx = torch.tensor(rows[gi])
            one = cpu_ops.fgfa_warp_aggregate(ring[idx], flows[gi * T:(gi + 1) * T], Cf, key_pos)
            assert torch.equal(got[gi], one)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", mc.CONV1_SHAPES)
def test_flow_conv1_combine_twin_window_mode_equals_key_mode(shape, dtype):
    S, h, w = shape
    ab0, bias = mc.conv1_inputs(S, h, w)
    nwin = S - 2
    for G in (1, 3):
        rows = mc.conv1_group_orders(S, G, nwin)
        assert all(r[0] not in r[1:] and len(set(r[1:])) == nwin for r in rows)
        ab = mc.nan_unused(ab0, {s for r in rows for s in r})
        got = cpu_ops.flow_conv1_combine(ab, bias, dtype, order=mc.orders_tensor(rows), nwin=nwin)
        assert tuple(got.shape) == (G * nwin, h, w, 64) and torch.isfinite(got.float()).all()
        for gi, r in enumerate(rows):
            gathered = torch.cat([ab[r[1:]], ab[r[0]:r[0] + 1]], dim=0)      # the window's frames, then the key frame
            one = cpu_ops.flow_conv1_combine(gathered, bias, dtype, key=nwin, T=nwin)
            assert torch.equal(got[gi * nwin:(gi + 1) * nwin].view(torch.int16), one.view(torch.int16))
    # order[0] mode == key mode
    a = cpu_ops.flow_conv1_combine(ab0, bias, dtype, order=mc.orders_tensor([3] + list(range(S))))
    b = cpu_ops.flow_conv1_combine(ab0, bias, dtype, key=3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_flow_pred_finish_twin_is_the_3x3_conv(scale):
    """z is the 1 x 1 conv of a level map x with the 18 (tap, channel) columns of a Conv2d(Cin, 2, 3, padding=1) weight: the
    twin's sum of the shifted taps is that 3 x 3 convolution; and the float64 reference agrees with the twin."""
    g = torch.Generator().manual_seed(7)
    N, H, W, Cin = 2, 6, 9, 24
    x = torch.randn((N, Cin, H, W), generator=g)
    wgt = torch.randn((2, Cin, 3, 3), generator=g) / 8
    bias = torch.randn((2,), generator=g)
    w18 = wgt.permute(2, 3, 0, 1).reshape(18, Cin)                      # row (r * 3 + s) * 2 + c
    z = torch.einsum("nchw,kc->nhwk", x, w18).contiguous()
    z = torch.cat([z, torch.full((N, H, W, 2), float("nan"))], dim=3)     # ldz = 20: the pad columns are not taps
    got = cpu_ops.flow_pred_finish(z, bias, scale, torch.float32)
    want = (F.conv2d(x, wgt, None, padding=1) * scale + bias.view(1, 2, 1, 1)).permute(0, 2, 3, 1)
    assert (got - want).abs().max() < 1e-5 * want.abs().max()
    ref, mag = mc.flow_pred_finish_f64(z, bias, scale)
    assert ((got.double() - ref).abs() <= 10 * 2.0 ** -24 * mag + mc.half_ulp(ref, torch.float32)).all()
    for dt, p in ((torch.float32, 24), (torch.bfloat16, 8), (torch.float16, 11)):      # half_ulp is the rounding's own bound
        r = ref.abs() * 0.37
        assert ((r.to(dt).double() - r).abs() <= mc.half_ulp(r, dt)).all() and (mc.half_ulp(r, dt) <= 2.0 ** -p * r).all()
        assert ((r.to(dt).double() - r).abs() > 0.9 * mc.half_ulp(r, dt)).any() or dt == torch.float32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_attention_and_position_f64_references_agree_with_the_twins(dtype):
    wg, bg, dim_mat = mc.attn_pos_weights()
    for shape in [(33, 97), (40, 70, 80), (1, 5)]:
        it = mc.attn_item(shape, dtype, seed=1)
        pos = cpu_ops.position_logits(it["rq"], it["rk"], wg, bg, dim_mat)
        twin = cpu_ops.relation_attention(it["q"], it["k"], it["vt"], it["Nk"], pos=pos, resid=it["resid"], bias_v=it["bias_v"])
        ref = mc.relation_attention_f64(it["q"], it["k"], it["vt"], it["Nk"], pos=pos, resid=it["resid"], bias_v=it["bias_v"])
        err = ((twin.double() - ref).abs().max() / ref.abs().max()).item()
        # f32: round-off of the f32 products; 16-bit: the rounding of e^(s - max) can flip on an f32 / f64 difference of the
        # scores (one operand ulp of one weight) + the twin's output rounding
        assert err < {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -9}[dtype], err
        if it["N2"]:       # the two-segment views hold the keys of the one-buffer form
            N1, N2, a, b = it["N1"], it["N2"], it["a_cols"], it["b_cols"]
            two = cpu_ops.relation_attention_batched([{
                "q": it["q"], "k": it["kb1"][2:2 + N1], "vt": it["big1"][:, a:a + N1], "N1": N1, "k2": it["kb2"][1:1 + N2],
                "vt2": it["big2"][:, b:b + N2], "Nk": it["Nk"], "pos": pos, "resid": it["resid"], "bias_v": it["bias_v"]}])[0]
            assert torch.equal(two, twin)


def test_position_f64_reference_agrees_with_the_f32_twin():
    """the float64 formula against the f32 twin (the exact formula in f32): 5e-4 on exp() at the problems the GPU module
    measures against float64 -- a twelfth of the fast kernel's bound -- and the cancellation of near-coincident centres at
    300 x 750 that keeps that problem out of the float64 comparison (see POS_F64_CHECKED)"""
    wg_t, bg, dim_mat = mc.pos_weights()
    assert all(p in mc.POS_PROBLEMS for p in mc.POS_F64_CHECKED) and len(mc.POS_F64_CHECKED) == 3
    for p in mc.POS_F64_CHECKED + [(300, 750)]:
        bq, bk = mc.pos_problem(*p)
        twin = cpu_ops.position_logits(bq, bk, wg_t, bg, dim_mat)[:, :, :p[1]]
        err = (twin.exp().double() - mc.position_logits_f64(bq, bk, wg_t, bg).exp()).abs()
        assert err.mean() < 1e-5
        assert (err.max() < 5e-4) == (p in mc.POS_F64_CHECKED), (p, err.max())


def test_case_tables():
    """the properties the GPU module relies on"""
    assert len({q for q, _ in mc.ATTN_CHUNK_ITEMS}) == 21 and len({k for _, k in mc.ATTN_CHUNK_ITEMS}) == 21
    assert min(q for q, _ in mc.ATTN_CHUNK_ITEMS) == 3 and max(q for q, _ in mc.ATTN_CHUNK_ITEMS) == 43
    assert min(k for _, k in mc.ATTN_CHUNK_ITEMS) == 5 and max(k for _, k in mc.ATTN_CHUNK_ITEMS) == 70
    assert len(mc.POS_CHUNK_PROBLEMS) == 23 and len(set(mc.POS_CHUNK_PROBLEMS)) == 23
    for S, T, _, _, _, _ in mc.FGFA_GEOMETRIES:
        assert mc.wrapped_slots(S, T)[:4] == [S - 2, S - 1, 0, 1]
        assert sorted(mc.shuffled_slots(S, T, 3)) != mc.shuffled_slots(S, T, 3) and len(set(mc.shuffled_slots(S, T, 3))) == T
        rows = mc.group_slots(S, T, 5)
        assert len({tuple(r) for r in rows}) == 5 and all(len(set(r)) == T for r in rows)
        assert set(rows[0]) & set(rows[1])
