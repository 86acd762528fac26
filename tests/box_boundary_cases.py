"""Deterministic inputs that sit ON the decision boundaries of csrc/boxes.hip (random inputs almost never do), each with the
facts it is meant to have, the oracle's answer, and the comparison helpers the GPU tests use.  CPU only: numpy, torch, the
oracle.  tests/test_box_boundary_cases.py proves the facts and that the helpers reject planted faults;
tests/test_box_boundary_gpu.py runs the kernels.

  band pairs   nested integer boxes whose IoU is within 1e-5 (relative) of the NMS threshold: the quotient path of
               dev_suppresses_areas.  All areas < 2^24: intersection, union and their operands are exact in f32, so the only
               rounding is the division's, and the decision is np.float32(I) / np.float32(U) against np.float32(thr).
  chains       boxes [i*shift, 0, i*shift + 99, 49], scores descending in i: the kept set is every second / third box, in
               closed form, and every box's fate depends on its predecessor's across 64-box blocks and 1024-box windows.
  RPN cases    logits with ties across the top-k cut, signed zeros, ulp ladders; deltas that decode (by construction) to boxes
               on a lattice whose IoUs are far from the threshold and whose sides are far from min_size, with clamped
               dw / dh, an all-invalid first block and one-pixel columns.
  post cases   ragged nprop with dead rows that must be ignored, exact score ties at the detections-per-image cut.

Margins: the device's expf differs from torch's by an ulp, so a decoded box moves around the 1e-4 level.  Every case that
goes through a decoder therefore measures, with the oracle, the smallest |side - min_size| over the decoded candidates and
the smallest |IoU - thr| over every pair the greedy pass compares, and reseeds itself until both are >= MARGIN.  NaN
scores are out of scope everywhere (no caller orders NaNs)."""
import collections
import functools
import math

import numpy as np
import torch

from oracle import mega_oracle as mo

BAND = 1e-5            # the relative half-width of dev_suppresses_areas' quotient band
MARGIN = 1e-3
CLIP = mo.BBOX_XFORM_CLIP
THRS = (0.3, 0.5, 0.7)
CLASSES = ("below", "equal", "above")
PER_CLASS = 64


# ===================================================================================================== band pairs
@functools.lru_cache(maxsize=None)
def band_pairs(thr):
    """{class: int64 [n][4] rows (W, H, w, h)}: box [0,0,w-1,h-1] nested in [0,0,W-1,H-1], |w*h - thr*W*H| within the band,
    classified by the f32 quotient against the f32 threshold.  (W in steps of 3: steps of 7 leave thr = 0.7 with 57 "equal"
    pairs, short of PER_CLASS.)"""
    t32 = np.float32(thr)
    found = {c: [] for c in CLASSES}
    for W in range(1500, 2001, 3):
        H = W - 3
        U = W * H
        w = np.arange(W // 2, W + 1, dtype=np.int64)
        hs = np.stack([np.floor(thr * U / w), np.ceil(thr * U / w)], 1).astype(np.int64)
        for col in (0, 1):
            h = hs[:, col]
            ok = (h >= 1) & (h <= H) & (np.abs(w * h - thr * U) <= BAND * thr * U)
            if col == 1:
                ok &= hs[:, 1] != hs[:, 0]
            for wi, hi in zip(w[ok], h[ok]):
                I = int(wi * hi)
                assert U + I < 1 << 24                      # Sa + Sb is exact too
                q = np.float32(I) / np.float32(U)
                found["below" if q < t32 else "above" if q > t32 else "equal"].append((W, H, int(wi), int(hi)))
    return {c: np.array(v, dtype=np.int64).reshape(-1, 4) for c, v in found.items()}


def quotient_class(pairs, thr):
    """-1 / 0 / +1 per pair: the f32 quotient below / equal to / above the f32 threshold."""
    q = (pairs[:, 2] * pairs[:, 3]).astype(np.float32) / (pairs[:, 0] * pairs[:, 1]).astype(np.float32)
    return np.sign(q.astype(np.float64) - float(np.float32(thr))).astype(np.int64)


def lay_out(pairs, seed=0):
    """The pairs on a grid of disjoint 2048 x 2048 cells (integer offsets < 2^20: every difference stays exact), the nested
    box with the lower score, rows shuffled.  -> boxes f32 [2n][4], scores f32 [2n], outer rows [n], inner rows [n]."""
    n = len(pairs)
    rng = np.random.RandomState(seed)
    ox, oy = (np.arange(n) % 256) * 2048, (np.arange(n) // 256) * 2048
    assert ox.max() + 2048 <= 1 << 20 and oy.max() + 2048 <= 1 << 20 and pairs[:, :2].max() <= 2000
    W, H, w, h = pairs.T
    boxes = np.concatenate([np.stack([ox, oy, ox + W - 1, oy + H - 1], 1), np.stack([ox, oy, ox + w - 1, oy + h - 1], 1)])
    scores = np.concatenate([2 * n - rng.permutation(n), n - rng.permutation(n)])          # outer n+1 .. 2n, inner 1 .. n
    perm = rng.permutation(2 * n)
    row_of = np.argsort(perm)
    return boxes[perm].astype(np.float32), scores[perm].astype(np.float32), row_of[:n], row_of[n:]


BandSet = collections.namedtuple("BandSet", "thr pairs cls boxes scores outer inner")


@functools.lru_cache(maxsize=None)
def band_set(thr, large):
    """small: PER_CLASS pairs of each class (384 boxes: the mask + scan form); large: the same pairs repeated in further
    cells up to 1100 pairs (2200 boxes: the lazy form)."""
    bp = band_pairs(thr)
    pairs = np.concatenate([bp[c][:PER_CLASS] for c in CLASSES])
    if large:
        pairs = np.concatenate([bp[c][:367] for c in CLASSES])
        pairs = pairs[np.arange(1100) % len(pairs)]
    boxes, scores, outer, inner = lay_out(pairs, seed=int(thr * 10) + 100 * large)
    return BandSet(thr, pairs, quotient_class(pairs, thr), boxes, scores, outer, inner)


def band_keep(bs, strict_gt):
    """The kept rows (ascending) that the quotient classes imply: every outer box, and the inner box unless suppressed."""
    sup = bs.cls > 0 if strict_gt else bs.cls >= 0
    return np.sort(np.concatenate([bs.outer, bs.inner[~sup]]))


# ===================================================================================================== chains
CHAIN_PERIOD = {(20, 0.5): 2, (10, 0.7): 2, (40, 0.3): 2, (20, 0.4): 3}       # (shift, thr) -> every period-th box is kept
CHAIN_N = (65, 1023, 1024, 1025, 2047, 2048, 2049, 2112, 3073)


def chain(n, shift, seed=0):
    """-> boxes f32 [n][4], scores f32 [n], rank [n]: row j holds the box of rank rank[j] (0 = best score).  shift = 100:
    all disjoint; shift = 0: all identical."""
    perm = np.random.RandomState(seed + n).permutation(n)
    i = perm.astype(np.int64)
    boxes = np.stack([i * shift, 0 * i, i * shift + 99, 0 * i + 49], 1).astype(np.float32)
    return boxes, (n - i).astype(np.float32), perm


def chain_keep(rank, period):
    """rows (ascending) of the boxes whose rank is a multiple of period; period = len(rank): only the best one"""
    return np.nonzero(rank % period == 0)[0].astype(np.int64)


# ===================================================================================================== greedy margin
def greedy_margin(boxes, thr, max_keep=None):
    """Greedy NMS in float64 over boxes in processing order -> (smallest |IoU - thr| over every pair it compares -- each kept
    box against the later boxes still alive --, kept count).  Stops, like the kernels, once max_keep boxes are kept."""
    b = boxes.double()
    n = b.shape[0]
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    alive = torch.ones(n, dtype=torch.bool)
    margin, kept = float("inf"), 0
    for i in range(n):
        if not alive[i]:
            continue
        kept += 1
        if (max_keep is not None and kept >= max_keep) or i + 1 == n:
            break
        r = b[i + 1:]
        iw = (torch.minimum(r[:, 2], b[i, 2]) - torch.maximum(r[:, 0], b[i, 0]) + 1).clamp(min=0)
        ih = (torch.minimum(r[:, 3], b[i, 3]) - torch.maximum(r[:, 1], b[i, 1]) + 1).clamp(min=0)
        iou = iw * ih / (area[i] + area[i + 1:] - iw * ih)
        live = alive[i + 1:]
        if live.any():
            margin = min(margin, float((iou[live] - thr).abs().min()))
        alive[i + 1:] = live & ~(iou > thr)
    return margin, kept


def all_pairs_margin(boxes, thr):
    """smallest |IoU - thr| over ALL pairs of the boxes: a superset of the pairs a greedy pass compares, in one matrix"""
    b = boxes.double()
    if b.shape[0] < 2:
        return float("inf")
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    iw = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0]) + 1).clamp(min=0)
    ih = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1]) + 1).clamp(min=0)
    iou = iw * ih / (area[:, None] + area[None, :] - iw * ih)
    iou.fill_diagonal_(thr + 1)
    return float((iou - thr).abs().min())


# ===================================================================================================== RPN cases
RPN_IM = 4096.0                     # large enough that a box clamped to 62.5 x the smallest anchor side stays inside
RpnSpec = collections.namedtuple("RpnSpec", "name Hf Wf k post min_size G logit delta")
# logit : ("ties", T, n_eq, take_eq, where) | ("equal", T) | ("zeros", n_neg, n_pos, take_eq) | ("ladder", base_bits, steps)
# G     : boxes per lattice cell, of which two survive NMS.  G = 3: post boxes are kept long before rank k (the max_keep stop);
#         larger G: fewer than post boxes survive, the walk reaches the last candidate and the ties at the cut show in the answer
# delta : subset of {"clamp", "block0", "column", "two_sizes"}
L1 = ("ladder", 0x3F800000, 256)    # 1.0 + j ulp, j < 256: 256 distinct keys that share their top three bytes
L2 = ("ladder", 0x3F7FFF00, 512)    # crosses 1.0: the second and third key bytes change inside the ladder
RPN_SPECS = [
    # 6 x 9 (NA = 648, one chunk), k < 1024: the mask + scan form
    RpnSpec("s-ties-1", 6, 9, 500, 63, 0, 24, ("ties", 0.75, 120, 1, "spread"), {"clamp", "column"}),
    RpnSpec("s-ties-half", 6, 9, 500, 63, 0, 24, ("ties", 0.75, 120, 60, "spread"), {"clamp", "column"}),
    RpnSpec("s-ties-all", 6, 9, 500, 63, 0, 24, ("ties", 0.75, 120, 120, "spread"), {"clamp", "column"}),
    RpnSpec("s-nocut-equal", 6, 9, 648, 300, 2, 12, ("equal", -1.5), {"block0", "column", "clamp"}),
    RpnSpec("s-nocut-zeros", 6, 9, 648, 300, 2, 12, ("zeros", 150, 150, 300), {"block0", "column", "clamp"}),
    RpnSpec("s-nocut-ladder", 6, 9, 648, 300, 2, 12, L1, {"block0", "column", "clamp"}),
    RpnSpec("s-post1", 6, 9, 500, 1, 0, 3, ("ties", -2.0, 200, 100, "spread"), {"clamp"}),
    RpnSpec("s-post65", 6, 9, 500, 65, 30, 3, ("zeros", 40, 40, 40), {"two_sizes", "clamp"}),
    # 10 x 16 (NA = 1920, two chunks), k = 1024, 4 * post <= k: the lazy form, one window
    RpnSpec("m-last-chunk", 10, 16, 1024, 64, 30, 64, ("ties", 0.5, 300, 150, "last"), {"two_sizes", "clamp"}),
    RpnSpec("m-negative-T", 10, 16, 1024, 64, 30, 64, ("ties", -3.25, 400, 200, "spread"), {"two_sizes", "clamp"}),
    RpnSpec("m-zeros", 10, 16, 1024, 64, 30, 64, ("zeros", 150, 250, 150), {"two_sizes", "clamp"}),
    # 10 x 16, k = 1100, 4 * post > k: the mask + scan form with 18 column blocks and invalid candidates
    RpnSpec("m-scan-ties", 10, 16, 1100, 300, 30, 12, ("ties", 1.25, 500, 250, "spread"), {"two_sizes", "column", "clamp"}),
    RpnSpec("m-scan-block0", 10, 16, 1100, 300, 2, 12, ("ties", 1.25, 500, 500, "spread"), {"block0", "column", "clamp"}),
    RpnSpec("m-scan-ladder2", 10, 16, 1100, 300, 2, 12, L2, {"block0", "column", "clamp"}),
    # 12 x 18 (NA = 2592, three chunks), k = 1200 = 4 * post: the lazy form, two windows
    RpnSpec("l-ties-1", 12, 18, 1200, 300, 2, 12, ("ties", 0.75, 600, 1, "spread"), {"block0", "column", "clamp"}),
    RpnSpec("l-ties-half", 12, 18, 1200, 300, 2, 12, ("ties", 0.75, 600, 300, "spread"), {"block0", "column", "clamp"}),
    RpnSpec("l-ladder", 12, 18, 1200, 300, 2, 3, L1, {"block0", "column", "clamp"}),
    RpnSpec("l-ladder2", 12, 18, 1200, 300, 2, 12, L2, {"block0", "column", "clamp"}),
    # 12 x 18, k = NA: no cut, three windows
    RpnSpec("l-nocut-equal", 12, 18, 2592, 65, 0, 96, ("equal", 2.0), {"clamp"}),
    RpnSpec("l-nocut-ties", 12, 18, 2592, 65, 0, 96, ("ties", -0.5, 500, 500, "last"), {"clamp"}),
    RpnSpec("l-nocut-zeros", 12, 18, 2592, 65, 0, 96, ("zeros", 400, 500, 900), {"clamp"}),
]
RPN_BY_NAME = {s.name: s for s in RPN_SPECS}


def rpn_batches():
    """specs that share one launch's parameters, three at a time: the B = 3 form"""
    groups = collections.OrderedDict()
    for s in RPN_SPECS:
        groups.setdefault((s.Hf, s.Wf, s.k, s.post, s.min_size), []).append(s.name)
    return [tuple(v[:3]) for v in groups.values() if len(v) >= 3]


def sortable_key(x):
    """numpy twin of box_math.h's f32_sortable: u32 keys whose order is the floats' order, -0.0 with +0.0's key"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def _logits(spec, NA, rng):
    kind = spec.logit[0]
    k = spec.k
    nchunk = (NA + 1023) // 1024
    if kind == "equal":
        return np.full(NA, spec.logit[1], dtype=np.float32)
    if kind == "ladder":
        base, steps = spec.logit[1:]
        j = rng.permutation(np.concatenate([np.arange(steps), rng.randint(0, steps, NA - steps)]))      # every step is held
        return (np.uint32(base) + j.astype(np.uint32)).view(np.float32)
    if kind == "ties":
        T, n_eq, take_eq, where = spec.logit[1:]
    else:
        n_neg, n_pos, take_eq = spec.logit[1:]
        T, n_eq, where = 0.0, n_neg + n_pos, "spread"
    if where == "last":
        eq = (nchunk - 1) * 1024 + rng.permutation(NA - (nchunk - 1) * 1024)[:n_eq]
    else:                                                   # every chunk holds its share of the ties
        eq = np.concatenate([c * 1024 + rng.permutation(min(1024, NA - c * 1024))[:(n_eq + c) // nchunk] for c in range(nchunk)])
    eq = np.sort(eq)
    assert len(eq) == n_eq
    n_gt = k - take_eq
    rest = rng.permutation(np.setdiff1d(np.arange(NA), eq))
    assert 0 <= n_gt <= len(rest)
    x = np.empty(NA, dtype=np.float32)
    x[rest[:n_gt]] = T + 0.25 + (1 + rng.permutation(n_gt)) * (2.0 / max(n_gt, 1))        # distinct, strictly greater
    x[rest[n_gt:]] = T - 0.25 - rng.rand(len(rest) - n_gt) * 3
    x[eq] = T
    if kind == "zeros":
        x[eq[:n_neg]] = -0.0                                # -0.0 at lower indices than +0.0
    return x


def _deltas(spec, order, anchors, rng):
    """The top-k anchors (by rank) decode to lattice boxes, G per cell: G - 1 of them the base box shifted along x by 0 .. 0.09
    side (IoU >= 0.8 with one another: the first in rank suppresses the rest) and one shifted along y by 0.4 side (IoU about 0.43
    with the base, below 0.4 with the others: kept), cells 96 px apart, ranks scattered over the cells.  Anchors outside the top-k are never decoded and hold noise."""
    NA, k = anchors.shape[0], len(order)
    reg = rng.randn(NA, 4) * 0.5
    a = anchors[order].double().numpy()
    aw, ah = a[:, 2] - a[:, 0] + 1, a[:, 3] - a[:, 1] + 1
    acx, acy = a[:, 0] + 0.5 * aw, a[:, 1] + 0.5 * ah
    slot = rng.permutation(k)
    G = spec.G
    cell, m = slot // G, slot % G
    ncell = (k + G - 1) // G
    ncol = int(math.ceil(math.sqrt(ncell)))
    x0 = RPN_IM / 2 - ncol * 96 / 2
    S = (np.where(rng.rand(ncell) < 0.5, 20.0, 40.0) if "two_sizes" in spec.delta else np.full(ncell, 40.0))[cell]
    cx = x0 + (cell % ncol) * 96 + 48 + np.where(m < G - 1, 0.015 * (m % 7) * S, 0) + rng.uniform(-0.25, 0.25, k)
    cy = x0 + (cell // ncol) * 96 + 48 + np.where(m == G - 1, 0.4 * S, 0) + rng.uniform(-0.25, 0.25, k)
    tw, th = S + rng.uniform(-0.25, 0.25, k), S + rng.uniform(-0.25, 0.25, k)
    d = np.stack([(cx - acx) / aw, (cy - acy) / ah, np.log(tw / aw), np.log(th / ah)], 1)
    free = np.arange(64, k)
    if "block0" in spec.delta:                              # the 64 best-ranked collapse: a whole first block is invalid
        d[:64, 2:] = -20.0
    if "column" in spec.delta:                              # far right of the image: clipped to the one-pixel column x = W - 1
        d[rng.choice(free, 8, replace=False), 0] = 100.0
    if "clamp" in spec.delta:                               # dw / dh above log(1000 / 16) on the narrowest / flattest anchors:
        for col, side, ctr in ((2, aw, acx), (3, ah, acy)):     # 62.5 x the side still fits the image, the unclamped box would not
            rows = free[(side[free] == side.min()) & (d[free, 0] != 100.0)][:2]
            d[rows, col] = (6.0, 10.0)[:len(rows)]
            d[rows, col - 2] = (RPN_IM / 2 - ctr[rows]) / side[rows]
    reg[order.numpy()] = d
    return reg.astype(np.float32)


class RpnCase(object):
    def __init__(self, spec, seed):
        self.spec, self.seed = spec, seed
        self.name, self.Hf, self.Wf, self.pre, self.post, self.min_size = spec.name, spec.Hf, spec.Wf, spec.k, spec.post, spec.min_size
        self.thr, self.im_w, self.im_h = 0.7, RPN_IM, RPN_IM
        self.cell = mo.generate_anchors(16)
        self.A = self.cell.shape[0]
        self.anchors = mo.grid_anchors(self.cell, self.Hf, self.Wf, 16)
        NA = self.anchors.shape[0]
        rng = np.random.RandomState(seed)
        self.logit = torch.from_numpy(_logits(spec, NA, rng))
        self.order = torch.sort(-self.logit, stable=True)[1][:self.pre]
        self.deltas = torch.from_numpy(_deltas(spec, self.order, self.anchors, rng))
        self.facts = self._facts()

    # the two layouts: the oracle's (A, H, W) / (4A, H, W) maps and the kernel's [H*W][5A] rows
    def obj(self):
        return self.logit.view(self.Hf, self.Wf, self.A).permute(2, 0, 1).contiguous()

    def reg(self):
        return self.deltas.view(self.Hf, self.Wf, self.A * 4).permute(2, 0, 1).contiguous()

    def rpn_out(self):
        hw = self.Hf * self.Wf
        return torch.cat([self.logit.view(hw, self.A), self.deltas.view(hw, self.A * 4)], 1).contiguous()

    def decoded(self, order):
        props = mo.clip_to_image(mo.box_decode(self.deltas[order], self.anchors[order], (1.0, 1.0, 1.0, 1.0)), self.im_w, self.im_h)
        return props, props[:, 2] - props[:, 0] + 1, props[:, 3] - props[:, 1] + 1

    def _facts(self):
        lg, k = self.logit, self.pre
        T = lg[self.order[-1]]
        eq = (lg == T).nonzero().squeeze(1)
        keys = sortable_key(lg.numpy())
        tkey = sortable_key(np.array([float(T)]))[0]
        props, ws, hs = self.decoded(self.order)
        valid = (ws >= self.min_size) & (hs >= self.min_size)
        iou_margin, kept = greedy_margin(props[valid], self.thr, self.post)
        unclamped = mo.clip_to_image(self._decode_unclamped(), self.im_w, self.im_h)
        return dict(
            n_gt=int((lg > T).sum()), n_eq=int(eq.numel()), take_eq=k - int((lg > T).sum()),
            tie_chunks=sorted(set((eq // 1024).tolist())), T=float(T),
            keys_sharing_top3=int(np.unique(keys[(keys >> 8) == (tkey >> 8)]).size),
            top3_prefixes=int(np.unique(keys >> 8).size),
            invalid_share=1.0 - float(valid.float().mean()), first_block_invalid=not bool(valid[:64].any()),
            clamped=int((self.deltas[self.order][:, 2:] > CLIP).sum()),
            clamp_visible=int(((unclamped - props).abs().max(1)[0] > 1).sum()),
            columns=int(((ws == 1) & (props[:, 0] == self.im_w - 1)).sum()),
            side_margin=float(torch.minimum((ws - self.min_size).abs(), (hs - self.min_size).abs()).min()),
            iou_margin=iou_margin, kept=kept)

    def _decode_unclamped(self):
        d, a = self.deltas[self.order].double(), self.anchors[self.order].double()
        w, h = a[:, 2] - a[:, 0] + 1, a[:, 3] - a[:, 1] + 1
        pcx, pcy = d[:, 0] * w + a[:, 0] + 0.5 * w, d[:, 1] * h + a[:, 1] + 0.5 * h
        pw, ph = d[:, 2].exp() * w, d[:, 3].exp() * h
        return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], 1).float()

    def reference(self, fault=None):
        """mo.rpn_select step by step (equal to it with fault=None), or with one planted fault: 'tie_reversed' (ties ordered
        by descending index), 'invalid_through' (the best-ranked invalid candidate is let through)."""
        order = self.order
        if fault == "tie_reversed":
            order = (self.logit.numel() - 1 - torch.sort(-self.logit.flip(0), stable=True)[1])[:self.pre]
        scores = self.logit[order].sigmoid()
        props, ws, hs = self.decoded(order)
        valid = (ws >= self.min_size) & (hs >= self.min_size)
        if fault == "invalid_through":
            valid[(~valid).nonzero()[0]] = True
        keep_small = valid.nonzero().squeeze(1)
        props, scores, order = props[keep_small], scores[keep_small], order[keep_small]
        keep = mo.nms_ordered(props, self.thr, True)[:self.post]
        return props[keep], scores[keep], order[keep]

    def oracle(self):
        return mo.rpn_select(self.obj(), self.reg(), self.anchors, self.im_w, self.im_h, self.pre, self.post, self.thr, self.min_size,
                             True, want_index=True)


@functools.lru_cache(maxsize=None)
def rpn_case(name):
    spec = RPN_BY_NAME[name]
    for seed in range(1000 + 7 * RPN_SPECS.index(spec), 1000 + 7 * RPN_SPECS.index(spec) + 40):
        case = RpnCase(spec, seed)
        f = case.facts
        cut_in_ties = f["take_eq"] < f["n_eq"] or spec.logit[0] != "ladder" or spec.k == case.logit.numel()
        if f["side_margin"] >= MARGIN and f["iou_margin"] >= MARGIN and cut_in_ties:     # (a ladder's cut: inside a tie group)
            return case
    raise AssertionError("%s: no seed meets the margins" % name)


def rpn_output(ref, post):
    """an oracle answer (boxes, scores, index) in the kernel's output form: (props [post][4], scores [post], count, index [post])"""
    b, s, i = ref
    n = b.shape[0]
    props, scores, index = torch.zeros(post, 4), torch.zeros(post), torch.full((post,), -1, dtype=torch.int32)
    props[:n], scores[:n], index[:n] = b, s, i.int()
    return props, scores, n, index


def check_rpn(got, want, what):
    """got: one frame of ops.rpn_select(want_index=True) on the CPU (props, scores, count, index); want: the oracle's answer.
    Count and kept anchor indices bit for bit, boxes within 1e-3, scores within 1e-6 (test_rpn_select's tolerances), the
    rows past the count zero with index -1."""
    props, scores, n, index = got
    wb, ws, wi = want
    n = int(n)
    assert n == wb.shape[0], "%s: kept %d vs oracle %d" % (what, n, wb.shape[0])
    assert torch.equal(index[:n].long(), wi.long()), "%s: kept anchor indices differ, first at row %d" % (
        what, int((index[:n].long() != wi.long()).nonzero()[0]))
    assert bool((index[n:] == -1).all()) and not bool(props[n:].any()) and not bool(scores[n:].any()), "%s: rows past the count" % what
    if n:
        assert float((props[:n] - wb).abs().max()) < 1e-3, "%s: boxes off by %g" % (what, float((props[:n] - wb).abs().max()))
        assert float((scores[:n] - ws).abs().max()) < 1e-6, "%s: scores off by %g" % (what, float((scores[:n] - ws).abs().max()))


def check_keep(got, want, what):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert np.array_equal(got, want), "%s: %d kept vs %d; rows only in got %s, only in want %s" % (
        what, len(got), len(want), np.setdiff1d(got, want)[:8].tolist(), np.setdiff1d(want, got)[:8].tolist())


# ===================================================================================================== post-processor cases
POST_IM = 3400.0
PostSpec = collections.namedtuple("PostSpec", "name R NC nprop max_det layout ties clamp")
# layout "pairs"   : random logits (score_thresh 0.001), proposals in pairs of IoU about 0.9 / 0.2 -> NMS decides
#        "disjoint": pairwise disjoint proposals, one class above score_thresh = 0.05 per row, distinct scores except for
#                    `ties` = (a, b): the rows ranked max_det - a .. max_det + b by score (1-based) share one logit row, so
#                    the max_det-th score is held a + b + 1 times and b of those lie past the cut
POST_SPECS = [
    PostSpec("R1-one", 1, 2, 1, 100, "pairs", None, False),
    PostSpec("R1-none", 1, 31, 0, 100, "pairs", None, False),
    PostSpec("R63-half", 63, 31, 31, 100, "pairs", None, True),
    PostSpec("R64-D-eq-max", 64, 2, 64, 64, "disjoint", None, False),
    PostSpec("R64-none", 64, 31, 0, 100, "pairs", None, False),
    PostSpec("R64-half", 64, 2, 32, 100, "pairs", None, False),
    PostSpec("R65-D-max+1", 65, 2, 65, 64, "disjoint", None, False),
    PostSpec("R65-D-max+1-tied", 65, 31, 65, 64, "disjoint", (0, 1), False),
    PostSpec("R65-half", 65, 31, 32, 64, "pairs", None, True),
    PostSpec("R65-full", 65, 31, 65, 64, "pairs", None, True),
    PostSpec("R65-none", 65, 31, 0, 64, "pairs", None, False),
    PostSpec("R300-tied", 300, 31, 300, 100, "disjoint", (3, 3), True),
    PostSpec("R300-nocut", 300, 31, 150, 0, "pairs", None, True),
    PostSpec("R300-one", 300, 2, 1, 100, "pairs", None, False),
    PostSpec("R300-nc2", 300, 2, 300, 100, "pairs", None, True),
    PostSpec("R300-nc2-none", 300, 2, 0, 100, "pairs", None, False),
    PostSpec("R300-nc2-half", 300, 2, 150, 100, "disjoint", (0, 40), False),
    PostSpec("R300-nc2-tied", 300, 2, 300, 100, "disjoint", (5, 5), False),
    PostSpec("R300-nc2-dead", 300, 2, 0, 100, "disjoint", None, False),
    PostSpec("R1024-full", 1024, 31, 1024, 300, "pairs", None, True),
    PostSpec("R1024-half", 1024, 31, 512, 300, "pairs", None, True),
    PostSpec("R1024-none", 1024, 31, 0, 300, "pairs", None, False),
    PostSpec("R1024-tied", 1024, 2, 512, 100, "disjoint", (10, 9), False),
]
POST_BY_NAME = {s.name: s for s in POST_SPECS}
# one launch each: ragged nprop, one image with 0, the images' other launch parameters equal
POST_BATCHES = [("R65-half", "R65-none", "R65-full"), ("R300-nc2", "R300-nc2-none", "R300-one"),
                ("R300-nc2-half", "R300-nc2-dead", "R300-nc2-tied"), ("R1024-half", "R1024-none", "R1024-full")]


class PostCase(object):
    weights = (10.0, 10.0, 5.0, 5.0)
    nms = 0.5

    def __init__(self, spec, seed):
        self.spec, self.seed = spec, seed
        self.name, self.R, self.NC, self.nprop, self.max_det = spec.name, spec.R, spec.NC, spec.nprop, spec.max_det
        self.im_w = self.im_h = POST_IM
        R, NC, n = self.R, self.NC, self.nprop
        rng = np.random.RandomState(seed)
        g = torch.Generator().manual_seed(seed)
        disjoint = spec.layout == "disjoint"
        self.score_thresh = 0.05 if disjoint else 0.001
        # proposals: 40 x 40 boxes in cells 100 px apart, 32 per row; "pairs": two per cell, 2 px (IoU 0.9) or 27 px (0.2) apart
        slot = torch.from_numpy(rng.permutation(R))
        cell, m = (slot, torch.zeros_like(slot)) if disjoint else (slot // 2, slot % 2)
        x1 = 100.0 + (cell % 32) * 100 + m * torch.where(cell % 2 == 0, 2.0, 27.0)
        y1 = 100.0 + (cell // 32) * 100.0
        self.props = torch.stack([x1, y1, x1 + 39, y1 + 39], 1).float() + (torch.rand((R, 4), generator=g) - 0.5) * 0.5
        self.deltas = torch.randn((R, NC * 4), generator=g) * 0.3
        if disjoint:
            main = 1 + torch.arange(R) % (NC - 1)
            level = torch.full((R,), -9.0)
            level[:n] = 2.0 + 4.0 * torch.from_numpy(rng.permutation(n)).float() / max(n, 1)      # distinct, 4 / n apart
            # two live terms per row (background 0, the main class `level`, the rest -30): with 30 EQUAL background terms the
            # f32 softmax sum depends on the summation order by up to 30 half-ulps in one direction, 1e-6 of a score near 1 --
            # that is the order of a sum, not a boundary, and would sit on the scores' 1e-6 tolerance
            self.logits = torch.full((R, NC), -30.0)
            self.logits[:, 0] = 0.0
            self.logits[torch.arange(R), main] = level
            if spec.ties:
                by_score = torch.sort(-level[:n], stable=True)[1]
                a, b = spec.ties
                rows = by_score[self.max_det - 1 - a:self.max_det + b]
                self.logits[rows] = self.logits[by_score[self.max_det - 1]].clone()
        else:
            self.logits = torch.randn((R, NC), generator=g) * 1.5
            main = self.logits[:, 1:].argmax(1) + 1
        self.clamp_rows = []
        if spec.clamp:      # dw above the clip on the best class of live rows near the centre: 62.5 x 40 px stays inside the image
            ok = ((self.props[:n, 0] > 1300) & (self.props[:n, 0] < 2100)).nonzero().squeeze(1)[:2]
            for r, v in zip(ok.tolist(), (30.0, 50.0)):
                self.deltas[r, main[r] * 4 + 2] = v
                self.clamp_rows.append(r)
        # the rows past nprop must be ignored: alternately NaN logits and a confident finite row, 1e30 deltas on both
        dead = torch.arange(n, R)
        self.logits[dead[0::2]] = float("nan")
        self.logits[dead[1::2]] = 0.0
        self.logits[dead[1::2], 1] = 8.0
        self.deltas[dead] = 1e30
        self.facts = self._facts()

    def cfg(self, **kw):
        return mo.OracleCfg(score_thresh=self.score_thresh, nms=self.nms, detections_per_img=self.max_det,
                            bbox_reg_weights=self.weights, num_classes=self.NC, **kw)

    def reference(self, fault=None):
        """mo.postprocess on the first nprop rows, or with one planted fault: 'cut_without_ties' (exactly max_det kept),
        'nprop_ignored' (every row with finite logits is live)."""
        n = self.nprop
        if fault == "nprop_ignored":
            live = torch.isfinite(self.logits).all(1).nonzero().squeeze(1)
            return mo.postprocess(self.logits[live], self.deltas[live].clamp(max=1e3), self.props[live], self.im_w, self.im_h, self.cfg())
        if n == 0:
            return torch.zeros((0, 4)), torch.zeros((0,)), torch.zeros((0,), dtype=torch.int64)
        b, s, l = mo.postprocess(self.logits[:n], self.deltas[:n], self.props[:n], self.im_w, self.im_h, self.cfg())
        if fault == "cut_without_ties" and self.max_det > 0 and s.numel() > self.max_det:
            keep = torch.sort(torch.sort(-s, stable=True)[1][:self.max_det])[0]
            b, s, l = b[keep], s[keep], l[keep]
        return b, s, l

    def _facts(self):
        n, NC = self.nprop, self.NC
        f = dict(D=0, kept=0, ties_at_cut=0, score_gap=float("inf"), thresh_margin=float("inf"), iou_margin=float("inf"),
                 clamped=len(self.clamp_rows), dead_nan=int(torch.isnan(self.logits).any(1).sum()),
                 dead_confident=int((self.logits[n:, 1] == 8.0).sum()) if NC > 1 else 0)
        if n == 0:
            return f
        lg, dl, pr = self.logits[:n], self.deltas[:n], self.props[:n]
        _, s_all, _ = mo.postprocess(lg, dl, pr, self.im_w, self.im_h, mo.OracleCfg(
            score_thresh=self.score_thresh, nms=self.nms, detections_per_img=0, bbox_reg_weights=self.weights, num_classes=NC))
        _, s, _ = self.reference()
        f["D"], f["kept"] = int(s_all.numel()), int(s.numel())
        if 0 < self.max_det < f["D"]:
            kth = torch.sort(s_all, descending=True)[0][self.max_det - 1]
            f["ties_at_cut"] = int((s_all == kth).sum())
            other = s_all[s_all != kth]
            if other.numel():
                f["score_gap"] = float((other - kth).abs().min())
        prob = torch.softmax(lg, -1)
        f["thresh_margin"] = float((prob[:, 1:] - self.score_thresh).abs().min())
        boxes = mo.clip_to_image(mo.box_decode(dl, pr, self.weights).reshape(-1, 4), self.im_w, self.im_h).reshape(n, NC * 4)
        for j in range(1, NC):
            inds = (prob[:, j] > self.score_thresh).nonzero().squeeze(1)
            if inds.numel() > 1:
                order = inds[torch.sort(-prob[inds, j], stable=True)[1]]
                f["iou_margin"] = min(f["iou_margin"], all_pairs_margin(boxes[order, j * 4:j * 4 + 4], self.nms))
        return f


@functools.lru_cache(maxsize=None)
def post_case(name):
    spec = POST_BY_NAME[name]
    base = 2000 + 11 * sorted(POST_BY_NAME).index(name)
    for seed in range(base, base + 40):
        case = PostCase(spec, seed)
        f = case.facts
        # (a probability moves by an ulp, about 1e-10 at score_thresh: 1e-8 is a hundred of them; the scores next to the
        # max_det-th one stay 1e-5 away from it, ten times the 1e-6 the scores are compared to)
        if f["iou_margin"] >= MARGIN and f["thresh_margin"] >= 1e-8 and f["score_gap"] >= 1e-5:
            return case
    raise AssertionError("%s: no seed meets the margins" % name)


def check_post(got, want, what):
    """got: (boxes, scores, labels, count) of ops.postprocess on the CPU; want: the oracle's (boxes, scores, labels).  Count and
    labels exact, boxes within 1e-3, scores within 1e-6 (test_postprocess's tolerances)."""
    ob, os_, ol, n = got
    wb, ws, wl = want
    n = int(n)
    assert n == wb.shape[0], "%s: %d detections vs oracle %d" % (what, n, wb.shape[0])
    if n:
        assert torch.equal(ol[:n], wl), "%s: labels differ" % what
        assert float((ob[:n] - wb).abs().max()) < 1e-3, "%s: boxes off by %g" % (what, float((ob[:n] - wb).abs().max()))
        assert float((os_[:n] - ws).abs().max()) < 1e-6, "%s: scores off by %g" % (what, float((os_[:n] - ws).abs().max()))
