"""Seeded inputs, ring / window tables and float64 references shared by tests/test_multi_launch_gpu.py (the batched, ring,
window-order and group forms of the kernels, on a GPU) and tests/test_multi_launch_twins.py (the same references checked
against each other on the CPU).  Not a test module: nothing here touches a device."""
import math

import torch
import torch.nn.functional as F

from oracle import mega_oracle as mo

# ------------------------------------------------------------------------------------------------ relation module
# (Nq, Nk) or (Nq, N1, N2) per problem of the heterogeneous attention launch, in launch order
ATTN_ITEMS = [(300, 750), (1, 5), (129, 64), (40, 1500), (257, 33), (33, 97), (40, 700, 800), (128, 31)]
# 21 one-segment problems, Nq over 3 .. 43 and Nk over 5 .. 70, all different: two launches of 11 and 10
ATTN_CHUNK_ITEMS = [(3 + 2 * i, 5 + (13 * i) % 66) for i in range(21)]
POS_PROBLEMS = [(37, 70), (5, 33), (300, 750), (64, 16), (1, 1), (9, 65), (8, 64)]
# 23 problems of distinct small sizes: two launches of 12 and 11
POS_CHUNK_PROBLEMS = [(1 + (7 * i) % 23, 2 + 3 * i) for i in range(23)]
# The problems whose logits are also measured against the float64 formula.  dx = log(|cx_q - cx_k| / w + 1e-3) cancels in f32
# when two centres nearly coincide, and the error is multiplied by 100 on its way into the sines: the exact f32 formula
# (cpu_ops.position_logits, libm sin / cos) is itself 4.8e-3 away from float64 on exp() at 300 x 750 (225 000 pairs, the closest
# centres 1e-3 of a box apart) -- most of the 6e-3 the fast kernel is allowed -- but at most 4.7e-4 on these three, which
# test_multi_launch_twins.py asserts.  (300, 750) is covered by the bit-equality with the single-problem kernel.
POS_F64_CHECKED = [(37, 70), (5, 33), (9, 65)]
ATTN_BOUND ={torch.float32: 2e-4, torch.bfloat16: 3e-2, torch.float16: 4e-3}   # test_relation_attention_hot_shapes


def boxes(g, n):
    """n boxes on a 900 x 500 canvas (the generator of test_position_logits_tiled_bf16)"""
    c = torch.rand((n, 2), generator=g) * torch.tensor([900., 500.])
    wh = torch.rand((n, 2), generator=g) * 250 + 2
    return torch.cat([c - wh / 2, c + wh / 2], dim=1)


def pos_problem(Nq, Nk):
    g = torch.Generator().manual_seed(Nq + Nk)
    b = boxes(g, Nq + Nk)
    return b[:Nq], b[Nq:]


def pos_weights():
    """(wg_t [64,16], bg [16], dim_mat [8]) of the seeded model's first local relation stage"""
    from mega.pytorch_amd import synth
    sd = synth.make_state_dict(blocks=(1, 1, 1), seed=4)
    w, bias = sd[mo.FE + "l_Wgs.0.weight"], sd[mo.FE + "l_Wgs.0.bias"]
    return w.view(16, 64).t().contiguous(), bias, mo.dim_mat_values()


def position_logits_f64(bq, bk, wg_t, bg):
    """cal_position_embedding -> conv -> relu -> + 1e-6 -> log in double: [16, Nq, Nk]"""
    pe = mo.cal_position_embedding(bq.double(), bk.double())
    w = wg_t.double().t().contiguous().view(16, 64, 1, 1)
    return (F.relu(F.conv2d(pe, w, bg.double())) + 1e-6).log()[0]


def attn_item(shape, dtype, seed, resid_dtype=None):
    """One attention problem on the CPU, built like test_attention_two_key_segments_bit_equal: q, the keys in ONE K / V^T
    buffer (k, vt: what the reference reads) and, for (Nq, N1, N2), the same keys as two segments inside wider buffers at odd
    element offsets (kb1 / big1 / kb2 / big2 with their offsets); its own resid and bias_v; the boxes of its position term."""
    Nq, N1 = shape[0], shape[1]
    N2 = shape[2] if len(shape) == 3 else 0
    Nk = N1 + N2
    g = torch.Generator().manual_seed(seed * 7919 + Nq * 3 + Nk)
    it = {"Nq": Nq, "Nk": Nk, "N1": N1, "N2": N2}
    it["q"] = (torch.randn((Nq, 1024), generator=g) * 0.3).to(dtype)
    kfull = (torch.randn((Nk, 1024), generator=g) * 0.3).to(dtype)
    vfull = (torch.randn((1024, Nk), generator=g) + 0.5).to(dtype)
    it["resid"] = torch.randn((Nq, 1024), generator=g).to(resid_dtype or dtype)
    it["bias_v"] = torch.randn((1024,), generator=g) * 0.1
    vt = torch.zeros((1024, (Nk + 31) // 32 * 32), dtype=dtype)
    vt[:, :Nk] = vfull
    it["k"], it["vt"] = kfull, vt
    rq = torch.rand((Nq, 4), generator=g) * 100
    rq[:, 2:] += rq[:, :2] + 5
    rk = torch.rand((Nk, 4), generator=g) * 100
    rk[:, 2:] += rk[:, :2] + 5
    it["rq"], it["rk"] = rq, rk
    if N2:
        a_cols, b_cols = 3, 5
        big1 = torch.full((1024, (a_cols + N1 + 9 + 7) // 8 * 8), 7.0, dtype=dtype)   # (first segment: 16-byte row pitch)
        big1[:, a_cols:a_cols + N1] = vfull[:, :N1]
        big2 = torch.full((1024, b_cols + N2 + 11), -3.0, dtype=dtype)
        big2[:, b_cols:b_cols + N2] = vfull[:, N1:]
        kb1 = torch.zeros((2 + N1 + 1, 1024), dtype=dtype)
        kb1[2:2 + N1] = kfull[:N1]
        kb2 = torch.zeros((1 + N2 + 3, 1024), dtype=dtype)
        kb2[1:1 + N2] = kfull[N1:]
        it.update(big1=big1, big2=big2, kb1=kb1, kb2=kb2, a_cols=a_cols, b_cols=b_cols)
    return it


def attn_pos_weights():
    """Wg / bg / dim_mat of the attention items' position term (as test_attention_two_key_segments_bit_equal)"""
    g = torch.Generator().manual_seed(11)
    wg = torch.randn((64, 16), generator=g) * 0.3
    bg = torch.randn((16,), generator=g) * 0.1 + 0.3
    return wg, bg, torch.full((8,), 1000.0).pow(torch.arange(8) / 8.0)


def relation_attention_f64(q, k, vt, Nk, pos=None, resid=None, bias_v=None, groups=16):
    """cpu_ops.relation_attention in double on the same operands: the 16-bit modes keep the rounding of P to the operand type
    (the PV product and the row sum see the rounded weights); nothing else is rounded.  -> f64 [Nq, groups * 64]"""
    Nq = q.shape[0]
    qh = q.double().view(Nq, groups, 64).permute(1, 0, 2)
    kh = k.double()[:Nk].view(Nk, groups, 64).permute(1, 0, 2)
    s = torch.bmm(qh, kh.transpose(1, 2)) / math.sqrt(64.0)
    if pos is not None:
        s = s + pos.double()[:, :, :Nk]
    if q.dtype in (torch.bfloat16, torch.float16):
        e = torch.exp(s - s.max(dim=2, keepdim=True).values).to(q.dtype).double()
        p = e / e.sum(dim=2, keepdim=True)
    else:
        p = F.softmax(s, dim=2)
    v = vt.double()[:, :Nk].reshape(groups, 64, Nk)
    o = torch.bmm(p, v.transpose(1, 2)).permute(1, 0, 2).reshape(Nq, groups * 64)
    if bias_v is not None:
        o = o + bias_v.double()
    if resid is not None:
        o = o + resid.double()
    return o


# ------------------------------------------------------------------------------------------------ FGFA ring / window / group
FGFA_GEOMETRIES = [(9, 5, 6, 7, 16, 8), (25, 21, 12, 17, 64, 128), (7, 7, 9, 13, 128, 32)]     # (S, T, H, W, Cf, Ce)


def wrapped_slots(S, T, start=None):
    """a window that wraps round the ring: [S-2, S-1, 0, 1, ...] by default"""
    start = S - 2 if start is None else start
    return [(start + t) % S for t in range(T)]


def shuffled_slots(S, T, seed):
    """T different slots of the ring in random order"""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(S, generator=g)[:T].tolist()


def order_row(slots, key_pos):
    """a table row of the ring forms: [slot of the key frame] + the slots of the window positions.  The window-order form
    takes the key frame's flow field from window position key_pos and its features from order[0]: the contract is
    order[0] == order[1 + key_pos], which this builder keeps."""
    return [slots[key_pos]] + list(slots)


def orders_tensor(rows):
    return torch.tensor(rows, dtype=torch.int32)


def group_slots(S, T, G):
    """G different windows on one ring: consecutive wrapped windows (neighbours share T - 1 slots) and, from the third key
    frame on, every other one a shuffled permutation of its window"""
    rows = []
    for gi in range(G):
        s = wrapped_slots(S, T, (S - 2 + gi) % S)
        if gi >= 2 and gi % 2 == 0:
            g = torch.Generator().manual_seed(100 + gi)
            s = [s[i] for i in torch.randperm(T, generator=g).tolist()]
        rows.append(s)
    return rows


def fgfa_flow(g, n, H, W):
    """n flow fields as in test_fgfa_warp_aggregate: random x 3, one near-zero field, one row pushed far outside the map"""
    flow = torch.randn((n, 2, H, W), generator=g) * 3
    flow[n // 2] *= 0.05
    flow[0, :, 0, :] = 50.0
    return flow


def fgfa_ring(geometry, dtype, seed=0):
    """-> (ring [S,H,W,Cf+Ce] of dtype, flow_by_slot f32 [S,2,H,W]), every slot finite"""
    S, T, H, W, Cf, Ce = geometry
    g = torch.Generator().manual_seed(S * H + seed)
    ring = torch.randn((S, H, W, Cf + Ce), generator=g).to(dtype)
    return ring, fgfa_flow(g, S, H, W)


def nan_unused(t, used):
    """a copy of the per-slot tensor t with every slot outside `used` filled with NaN"""
    out = t.clone()
    for s in range(t.shape[0]):
        if s not in used:
            out[s] = float("nan")
    return out


def fgfa_aggregate_f64(ring, flow, slots, key_pos, Cf):
    """mo.fgfa_aggregate in double on the window's frames in window order (flow already in window order)
    -> (out f64 [H,W,Cf], weights f64 [T,H,W])"""
    idx = torch.tensor(slots, dtype=torch.long)
    feats = ring.index_select(0, idx).double().permute(0, 3, 1, 2)
    out, w = mo.fgfa_aggregate(feats, flow.double(), key_pos, nfeat=Cf)
    return out[0].permute(1, 2, 0).contiguous(), w[:, 0]


# ------------------------------------------------------------------------------------------------ FlowNetS pieces
CONV1_SHAPES = [(6, 5, 7), (23, 9, 11)]                                    # (S, h, w)
PRED_SHAPES = [(1, 1, 1, 18), (2, 3, 5, 18), (3, 7, 9, 64), (2, 1, 13, 20)]   # (N, H, W, ldz)


def half_ulp(ref, dtype):
    """half an ulp of `dtype` at |ref| (f64 tensor): 2^-p of the binade's lower end with p = 24 / 8 / 11 significant bits for
    f32 / bf16 / f16 (never more than 2^-24 / 2^-8 / 2^-11 of |ref|), half the smallest subnormal below the normal range"""
    p = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}[dtype]
    fi = torch.finfo(dtype)
    _, e = torch.frexp(ref.abs().clamp(min=fi.tiny))          # |ref| = m 2^e, m in [0.5, 1): the binade starts at 2^(e - 1)
    return torch.ldexp(torch.ones_like(ref), e - 1 - p)


def conv1_inputs(S, h, w, seed=0):
    """-> (ab f32 [S,h,w,128], bias f32 [64]); values of both signs so the leaky branch is taken about half the time"""
    g = torch.Generator().manual_seed(S * 131 + h * w + seed)
    return torch.randn((S, h, w, 128), generator=g), torch.randn((64,), generator=g) * 0.5


def conv1_group_orders(S, G, nwin, seed=0):
    """[G, 1 + nwin] rows [key slot, slots of the window]: the first window wraps round the ring, the others are shuffled
    permutations; every key slot lies OUTSIDE its own window (needs nwin < S)"""
    rows = []
    for gi in range(G):
        win = wrapped_slots(S, nwin) if gi == 0 else shuffled_slots(S, nwin, seed + 31 * gi)
        key = [s for s in range(S) if s not in win][gi % (S - nwin)]
        rows.append([key] + win)
    return rows


def pred_inputs(N, H, W, ldz, seed=0):
    """-> (z f32 [N,H,W,ldz], bias f32 [2]): columns 18 .. ldz-1 hold NaN, image n is 16^n times as large as image 0 (a row
    of a neighbouring image leaking into a sum is 16 x or 1 / 16 of the sum's own size; 256 x 9 taps x 2.5 still fits f16)"""
    g = torch.Generator().manual_seed(N * 1000 + H * 37 + W + seed)
    z = torch.randn((N, H, W, ldz), generator=g)
    z = z * torch.tensor([16.0 ** n for n in range(N)]).view(N, 1, 1, 1)
    z[..., 18:] = float("nan")
    return z, torch.randn((2,), generator=g)


def flow_pred_finish_f64(z, bias, scale):
    """the nine shifted taps with zero padding, * scale + bias, in double -> (ref f64 [N,H,W,2], mag f64 [N,H,W,2]) with
    mag = (sum of |taps|) * |scale| + |bias|: what the f32 round-off of the sum scales with"""
    N, H, W, _ = z.shape
    zp = F.pad(z[..., :18].double(), (0, 0, 1, 1, 1, 1))
    acc = torch.zeros((N, H, W, 2), dtype=torch.float64)
    mag = torch.zeros((N, H, W, 2), dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            tap = zp[:, r:r + H, s:s + W, (r * 3 + s) * 2:(r * 3 + s) * 2 + 2]
            acc = acc + tap
            mag = mag + tap.abs()
    b = bias.double().view(1, 1, 1, 2)
    return acc * scale + b, mag * abs(scale) + b.abs()
