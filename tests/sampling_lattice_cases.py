"""Deterministic inputs on which the kernels that turn a coordinate into a weighted gather -- ROIAlign, the two pools
(csrc/spatial.hip) and the two flow warps (csrc/fgfa.hip) -- have ONE right answer whatever the order of their sums, each
with a plain float64 restatement of the operation, a census of the decision boundaries its samples sit on and the comparison
helpers the GPU tests use.  CPU only: numpy, torch, the oracle.  tests/test_sampling_lattice_cases.py proves the facts and
that the helpers reject planted faults; tests/test_sampling_lattice_gpu.py runs the kernels.

  ROIAlign     spatial_scale = 1 / 16, integer features in [-8, 8].  A ROI of side P g 16 px (P = pooled size, g an integer)
               has bin_size = g and grid = g: its samples are start + 1/2 + j, j < P g, per axis.  With the corner on the 8 px
               lattice every sample sits on an integer or a half-integer, every bilinear weight is 0, 1/2 or 1 and every
               partial sum is exact in f32.  g in (1, 2, 4, 8): the count g g is a power of two, the quotient is exact too
               (the EXACT class: bit for bit).  g in (3, 5, 6, 7, 9, 11): only the final / count rounds (the ONE-ULP class).
               sampling_ratio = 2 with side P m 8 px: samples on eighths, count 4: exact.
               The corners put first / last samples ON -1, 0, N - 1 and N (kept and clamped), half a cell beyond (skipped)
               and inside; `census` counts them and derives the separable kernel's patch extents.
  ceil ladder  the exact ROI of height 7 g 16 and the same ROI with y2 one f32 step up / down: grid counts g, g + 1, g.
  pools        integer maps: max is a selection, the 2 x 2 ceil-mode average divides by 1, 2 or 4.
  warps        maps with W - 1 and H - 1 powers of two, flows on the 1/4 lattice: every coordinate, weight and blend is exact.

Non-finite values, ROIs in general position within an ulp of -1 or N, and 1-pixel-wide warp maps are out of scope."""
import collections
import functools
import math

import numpy as np
import torch

SCALE = 1.0 / 16
MAP_H, MAP_W, MAP_B = 24, 40, 3
EXACT_GS = (1, 2, 4, 8)
ULP_GS = (3, 5, 6, 7, 9)
OVERSIZE_G = 11                     # 121 samples per bin: not a power of two, so it lives in the one-ulp class
RATIO_MS = (1, 2, 3, 5, 8)
KINDS = ("on-1", "on0", "onN-1", "onN", "below", "above", "inside")
BOUNDARY_KEYS = ("at_m1", "at_0", "at_nm1", "at_n", "below", "above")


# ===================================================================================================== features
@functools.lru_cache(maxsize=None)
def int_features(B, H, W, C, seed=0):
    """f32 NHWC [B][H][W][C], integers in [-8, 8], drawn independently per element: no channel block is tiled, so a wrong
    channel-slice or image index reads different numbers (test_sampling_lattice_cases.py checks that no two (image, channel)
    planes are equal)."""
    rng = np.random.RandomState(1000 + seed)
    return torch.from_numpy(rng.randint(-8, 9, size=(B, H, W, C)).astype(np.float32))


# ===================================================================================================== ROI sets
def _axis_starts(first_off, last_off, n):
    """start coordinates (feature cells) of the seven kinds along an axis of n cells; first_off / last_off: the first and the
    last sample's offset from the start"""
    return {"on-1": -1.0 - first_off, "on0": 0.0 - first_off, "onN-1": (n - 1.0) - last_off, "onN": float(n) - last_off,
            "below": -1.5 - first_off, "above": (n + 0.5) - last_off, "inside": 1.0}


def _kind_rois(first_off, last_off, side, H, W, b0, B):
    """seven ROIs (rows b, x1, y1, x2, y2 in pixels): kind i along x with kind i + 3 along y, so each axis sees every kind"""
    sx, sy = _axis_starts(first_off, last_off, W), _axis_starts(first_off, last_off, H)
    rows = []
    for i, kx in enumerate(KINDS):
        ky = KINDS[(i + 3) % len(KINDS)]
        x1, y1 = sx[kx] * 16, sy[ky] * 16
        rows.append([(b0 + i) % B, x1, y1, x1 + side * 16, y1 + side * 16])
    return rows


def _tail_rois(P, H, W, n, B):
    """appended to every set: an inverted ROI (fmaxf(., 1) takes over: bin_size 1 / P, exact for P a power of two only), a ROI
    whose every sample lies right of and below the map, and one that misses the map along x alone"""
    rows = []
    if P in (4, 8):
        rows.append([n % B, 200.0, 120.0, 120.0, 40.0])
    rows.append([(n + 1) % B, (W + 2) * 16.0, (H + 2) * 16.0, (W + 2 + P) * 16.0, (H + 2 + P) * 16.0])
    rows.append([(n + 2) % B, (W + 2) * 16.0, 16.0, (W + 2 + P) * 16.0, (1 + P) * 16.0])
    return rows


@functools.lru_cache(maxsize=None)
def roi_lattice(P, gs, H=MAP_H, W=MAP_W, B=MAP_B):
    """f32 [K][5] for the adaptive grid (sampling_ratio 0): per g seven ROIs of side P g 16 px with corners on the 8 px
    lattice, then the tail.  'inside' starts on a whole cell (samples on half-integers, weights 1/2), the other kinds half a
    cell off (samples on integers)."""
    rows = []
    for g in gs:
        rows += _kind_rois(0.5, P * g - 0.5, P * g, H, W, len(rows), B)
    rows += _tail_rois(P, H, W, len(rows), B)
    rois = np.array(rows, dtype=np.float32)
    assert np.array_equal(rois[:, 1:] % 8, np.zeros_like(rois[:, 1:]))
    return torch.from_numpy(rois)


@functools.lru_cache(maxsize=None)
def oversize_roi(P, H=MAP_H, W=MAP_W):
    """one ROI with g = 11 (a 12-cell patch per bin: wider than the separable kernel's 10-slot tables), partly outside"""
    side = P * OVERSIZE_G
    return torch.tensor([[1.0, -4.5 * 16, 0.5 * 16, (-4.5 + side) * 16, (0.5 + side) * 16]], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def ulp_set(P, H=MAP_H, W=MAP_W, B=MAP_B):
    """the one-ulp class: g in ULP_GS plus the oversize ROI"""
    return torch.cat([roi_lattice(P, ULP_GS, H, W, B), oversize_roi(P, H, W)])


@functools.lru_cache(maxsize=None)
def ratio_lattice(P, ms=RATIO_MS, H=MAP_H, W=MAP_W, B=MAP_B):
    """f32 [K][5] for sampling_ratio = 2: side P m 8 px, bin_size m / 2, a bin's two samples at m / 8 and 3 m / 8"""
    rows = []
    for m in ms:
        rows += _kind_rois(m / 8.0, P * m / 2.0 - m / 8.0, P * m / 2.0, H, W, len(rows), B)
    rows += _tail_rois(P, H, W, len(rows), B)
    rois = np.array(rows, dtype=np.float32)
    assert np.array_equal(rois, np.round(rois))
    return torch.from_numpy(rois)


def repeat_to(rois, K):
    """the set repeated (or cut) to exactly K rows"""
    return rois[torch.arange(K) % rois.shape[0]].contiguous()


def f32_grid(y1, y2, P):
    """the kernels' expression for the adaptive grid count, in numpy f32"""
    s = np.float32(SCALE)
    h = np.maximum(np.float32(y2) * s - np.float32(y1) * s, np.float32(1.0))
    return int(np.ceil(h / np.float32(P)))


Ladder = collections.namedtuple("Ladder", "rois grids g kind")


@functools.lru_cache(maxsize=None)
def ceil_ladder(P=7):
    """per g in 1..8 three ROIs: height 7 g 16 px exactly, y2 one f32 step up, one step down (y1 = 8 px: half a cell, in y2's
    binade, so the step survives the subtraction -- and the bins straddle the cell borders: inside one cell the bilinear blend is
    linear and the mean over g + 1 samples would equal the mean over g); width 2 P 16 on the lattice.  grids: what f32_grid gives for each; kind: 'exact', 'up' (the bumped member: its
    grid count is g + 1 and its samples are in general position) or 'down' (grid g, every sample within an ulp of the lattice)."""
    rows, grids, gs, kind = [], [], [], []
    for g in range(1, 9):
        y2 = np.float32(P * g * 16 + 8)
        x1 = np.float32(8 * g)
        for j, yy in enumerate((y2, np.nextafter(y2, np.float32(np.inf)), np.nextafter(y2, np.float32(-np.inf)))):
            rows.append([(g + j) % MAP_B, x1, 8.0, x1 + 2 * P * 16, yy])
            grids.append(f32_grid(8.0, yy, P))
            gs.append(g)
            kind.append(("exact", "up", "down")[j])
    return Ladder(torch.from_numpy(np.array(rows, dtype=np.float32)), tuple(grids), tuple(gs), tuple(kind))


# ===================================================================================================== the float64 restatement
FAULTS = ("skip_at_n", "skip_at_m1", "collapsed_row_weight", "grid_floor_plus_1", "batch_ignored")


def _axis_sample(p, n, fault=None):
    """one sample along an axis of n cells -> (low, high, weight of low, weight of high), weights 0 when it is skipped"""
    if p < -1.0 or p > n or (fault == "skip_at_n" and p == n) or (fault == "skip_at_m1" and p == -1.0):
        return 0, 0, 0.0, 0.0
    if p <= 0:
        p = 0.0
    lo = int(p)
    if lo >= n - 1:
        if fault == "collapsed_row_weight":         # the collapsed pair keeps 1 - l of the sample it was given
            return n - 1, n - 1, 1.0 - min(p - (n - 1), 1.0), 0.0
        return n - 1, n - 1, 1.0, 0.0
    return lo, lo + 1, 1.0 - (p - lo), p - lo


def _roi_geometry(roi, P, ratio, fault=None, grid=None):
    """per axis (x, y): start, bin size and grid count of one ROI, in float64 from the f32 row"""
    out = []
    for a in (1, 2):
        start, end = float(roi[a]) * SCALE, float(roi[a + 2]) * SCALE
        size = max(end - start, 1.0)
        if ratio > 0:
            g = ratio
        elif fault == "grid_floor_plus_1":
            g = int(math.floor(size / P)) + 1
        else:
            g = int(math.ceil(size / P))
        if grid is not None and a == 2:
            g = grid
        out.append((start, size / P, g))
    return out


def _axis_matrix(start, bin_size, g, P, n, fault):
    m = np.zeros((P, n), dtype=np.float64)
    for p in range(P):
        for i in range(g):
            lo, hi, wl, wh = _axis_sample(start + p * bin_size + (i + 0.5) * bin_size / g, n, fault)
            m[p, lo] += wl
            m[p, hi] += wh
    return m


def roi_align_f64(feat_nhwc, rois, P, ratio=0, fault=None, grid_h=None, divide=True):
    """ROIAlign restated in float64: out[k][ph PW + pw][c] = (1 / count) sum over the bin's samples of the bilinear blend.  The
    per-axis weights are gathered into one matrix per axis (a sum of exact terms has no order).  fault: one of FAULTS;
    grid_h: the sampling grid's row count, forced; divide=False: the sums before the division.  -> float64 [K][P P][C]"""
    f = feat_nhwc.double().numpy()
    B, H, W, C = f.shape
    out = np.zeros((len(rois), P * P, C), dtype=np.float64)
    for k, roi in enumerate(rois.numpy()):
        b = 0 if fault == "batch_ignored" else int(roi[0])
        (sx, bx, gx), (sy, by, gy) = _roi_geometry(roi, P, ratio, fault, grid_h)
        wy, wx = _axis_matrix(sy, by, gy, P, H, fault), _axis_matrix(sx, bx, gx, P, W, fault)
        v = np.einsum("py,yxc->pxc", wy, f[b])
        out[k] = (np.einsum("qx,pxc->pqc", wx, v) / (float(gx * gy) if divide else 1.0)).reshape(P * P, C)
    return out


def oracle_roi_align(feat_nhwc, rois, P, ratio=0):
    """oracle.native.roi_align in the kernels' hot layout: f32 NHWC in, f32 [K][P P][C] out"""
    from oracle import native
    o = native.roi_align(feat_nhwc.permute(0, 3, 1, 2).contiguous().numpy(), rois.numpy(), SCALE, P, P, ratio)
    K, C = o.shape[:2]
    return torch.from_numpy(o).permute(0, 2, 3, 1).reshape(K, P * P, C).contiguous()


# ===================================================================================================== census
def census(rois, P, H, W, ratio=0):
    """A restatement of the sample geometry in plain Python.  -> (counts, patches): counts[axis] ('x' / 'y') = how many
    samples sit on exactly -1, 0, N - 1 and N and how many lie below -1 / above N (skipped); patches = per ROI (NR, NCm),
    the largest row / column count of a bin's touched patch, as roi_align_nhwc_sep_kernel's `table` derives it (0: empty)."""
    counts = {a: dict.fromkeys(BOUNDARY_KEYS, 0) for a in "xy"}
    patches = []
    for roi in rois.numpy():
        ext = []
        for name, n, (start, bs, g) in zip("xy", (W, H), _roi_geometry(roi, P, ratio)):
            c, widest = counts[name], 0
            for p in range(P):
                first, last = n, -1
                for i in range(g):
                    s = start + p * bs + (i + 0.5) * bs / g
                    c["at_m1"] += s == -1.0
                    c["at_0"] += s == 0.0
                    c["at_nm1"] += s == n - 1
                    c["at_n"] += s == n
                    c["below"] += s < -1.0
                    c["above"] += s > n
                    lo, hi, wl, wh = _axis_sample(s, n)
                    if wl + wh > 0:
                        first, last = min(first, lo), max(last, hi)
                widest = max(widest, last - first + 1 if last >= first else 0)
            ext.append(widest)
        patches.append((ext[1], ext[0]))
    return counts, patches


def ncm_class(ncm):
    """the column-count dispatch of roi_align_nhwc_sep_kernel (NC = 3, 4, 6, 10, the sample-by-sample fallback)"""
    return "empty" if ncm == 0 else "<=3" if ncm <= 3 else "4" if ncm == 4 else "5-6" if ncm <= 6 else "7-10" if ncm <= 10 else ">10"


# ===================================================================================================== the launch table
def roi_align_form(dtype, C, K, P, ratio, in_nhwc=True, out_nhwc=True):
    """which kernel mega_roi_align_fwd launches, restated from its thresholds (no test inspects the binary)"""
    ve = 4 if dtype == torch.float32 else 8
    if not (in_nhwc and out_nhwc and C % ve == 0):
        return "generic/%d" % (256 if C >= 256 else 128 if C >= 128 else 64)
    cv = C // ve
    slices = cv % 8 == 0 and cv // 8 >= 16
    if dtype != torch.float32 and ratio <= 0 and P <= 8:
        return "sep8" if slices else "sep1"
    return "vec-sliced" if slices and K * P * P * cv // 8 >= 256 * 64 else "vec"


def roi_align_planes_form(C, K, P, ratio):
    """the same for mega_roi_align_fwd_planes_dt"""
    cv = C // 4
    sliced = cv % 8 == 0 and cv // 8 >= 16 and K * P * P * cv // 8 >= 256 * 64
    return "sep8-planes" if sliced and ratio <= 0 and P <= 8 else "vec-sliced-planes" if sliced else "vec-planes"


# ===================================================================================================== pools
POOL_SIDES = (1, 2, 3, 5, 6, 7, 8)
POOL_BIG = (4, 301, 501, 64)        # N Ho Wo C / 4 = 2,425,664 work items (f32) > 8192 blocks x 256: the grid-stride loop iterates


def pool_cases():
    """(name, f32 NHWC map) with integer values in [-8, 8]: every pair of sides from {1, 2, 3, odd, even} with C = 8 and 64
    alternating, N = 2; 'neg-*' maps are all-negative (a pad read as 0 would win the max / shift the mean).  Both pools cap
    their grid at 8192 blocks of 256 one-vector items: POOL_BIG (through `pool_big`) is the one case past that."""
    rng = np.random.RandomState(77)
    i = 0
    for H in POOL_SIDES:
        for W in POOL_SIDES:
            C = (8, 64)[i % 2]
            i += 1
            yield "%dx%dx%d" % (H, W, C), torch.from_numpy(rng.randint(-8, 9, size=(2, H, W, C)).astype(np.float32))
    for H, W, C in ((1, 1, 8), (3, 5, 8), (6, 7, 64), (2, 2, 8)):
        yield "neg-%dx%dx%d" % (H, W, C), torch.from_numpy(rng.randint(-8, 0, size=(2, H, W, C)).astype(np.float32))


def pool_big():
    g = torch.Generator().manual_seed(78)
    return torch.randint(-8, 9, POOL_BIG, generator=g, dtype=torch.int8).float()


def pool_work_items(shape, ve, kind):
    """one-vector work items of the pool launch (compare with 8192 * 256)"""
    N, H, W, C = shape
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if kind == "max" else ((H + 1) // 2, (W + 1) // 2)
    return N * Ho * Wo * (C // ve)


# ===================================================================================================== warps
WARP_MAPS = ((3, 5), (5, 9), (9, 17), (17, 33))
WARP_FIELDS = ("mixed", "far", "zero", "whole", "mixed2")          # five fields: the T = 5 frames of the FGFA cases
WARP_KEY = WARP_FIELDS.index("zero")


def _unnormalised(p, f, n):
    """the kernels' sample coordinate before the border clamp, in numpy f32, operation by operation"""
    one, two = np.float32(1), np.float32(2)
    g = (np.float32(p) + np.float32(f)) / (np.float32(n - 1) / two) - one
    return ((g + one) * np.float32(n) - one) / two


def whole_pixel_flows(n):
    """{p: the flows f on the 1/4 lattice, |f| <= n, for which pixel p samples a whole pixel strictly inside 0 .. n - 1}, found
    by search with the f32 expression"""
    found = {}
    for p in range(n):
        fs = [q / 4.0 for q in range(-4 * n, 4 * n + 1)
              if float(_unnormalised(p, q / 4.0, n)) == math.floor(float(_unnormalised(p, q / 4.0, n)))
              and 0 < float(_unnormalised(p, q / 4.0, n)) < n - 1]
        if fs:
            found[p] = fs
    return found


@functools.lru_cache(maxsize=None)
def warp_lattice(H, W, seed=0):
    """f32 [5][2][H][W] (fields in WARP_FIELDS order), every value a multiple of 1/4:
      mixed / mixed2  random in [-3, 3]; the first / last row and column pushed beyond their border by more than the map size
      far             every pixel pushed out: one quadrant per corner
      zero            the identity warp (the FGFA key frame's field)
      whole           random, with the searched whole-pixel flows on every second pixel of an axis"""
    rng = np.random.RandomState(300 + 7 * seed + H)
    draw = lambda: rng.randint(-12, 13, size=(2, H, W)).astype(np.float32) / 4                  # noqa: E731
    out = {}
    for name in ("mixed", "mixed2"):
        f = draw()
        f[1, 0, :] = -(H + 2.25)
        f[1, H - 1, :] = H + 2.5
        f[0, :, 0] = -(W + 2.75)
        f[0, :, W - 1] = W + 2.0
        out[name] = f
    f = draw()
    f[0, :, :W // 2] -= 2 * W
    f[0, :, W // 2:] += 2 * W
    f[1, :H // 2, :] -= 2 * H
    f[1, H // 2:, :] += 2 * H
    out["far"] = f
    out["zero"] = np.zeros((2, H, W), dtype=np.float32)
    f = draw()
    wx, wy = whole_pixel_flows(W), whole_pixel_flows(H)
    assert wx and wy, "no whole-pixel flow on the 1/4 lattice for a %d x %d map" % (H, W)
    for px, fs in wx.items():
        f[0, px % 2::2, px] = fs[px % len(fs)]
    for py, fs in wy.items():
        f[1, py, py % 2::2] = fs[py % len(fs)]
    out["whole"] = f
    flows = np.stack([out[n] for n in WARP_FIELDS])
    assert np.array_equal(flows * 4, np.round(flows * 4))
    return torch.from_numpy(flows)


def warp_census(flow, H, W):
    """one field [2][H][W] -> samples clamped on the left / right / top / bottom and samples on whole pixels (x, y)"""
    xs = np.array([[float(_unnormalised(px, flow[0, py, px], W)) for px in range(W)] for py in range(H)])
    ys = np.array([[float(_unnormalised(py, flow[1, py, px], H)) for px in range(W)] for py in range(H)])
    inside = lambda v, n: (v > 0) & (v < n - 1) & (v == np.floor(v))                             # noqa: E731
    return dict(left=int((xs < 0).sum()), right=int((xs > W - 1).sum()), top=int((ys < 0).sum()), bottom=int((ys > H - 1).sum()),
                whole_x=int(inside(xs, W).sum()), whole_y=int(inside(ys, H).sum()))


def warp_f64(feats_hwc, flow, fault=None):
    """grid_sample(bilinear, border, align_corners=False) on the flow grid, restated in float64 -> float64 [H][W][C].
    fault 'clamp_before_unnormalise': the normalised coordinate is clamped to [-1, 1] and taps beyond the map read 0."""
    f = feats_hwc.double().numpy()
    H, W, C = f.shape
    fl = flow.double().numpy()
    out = np.zeros((H, W, C), dtype=np.float64)
    tap = lambda y, x: f[y, x] if 0 <= y < H and 0 <= x < W else 0.0                              # noqa: E731
    for py in range(H):
        for px in range(W):
            c = []
            for p, d, n in ((px, fl[0, py, px], W), (py, fl[1, py, px], H)):
                g = (p + d) / ((n - 1) / 2.0) - 1.0
                if fault == "clamp_before_unnormalise":
                    g = min(max(g, -1.0), 1.0)
                i = ((g + 1.0) * n - 1.0) / 2.0
                if fault is None:
                    i = min(max(i, 0.0), n - 1.0)
                c.append(i)
            x0, y0 = int(math.floor(c[0])), int(math.floor(c[1]))
            wx, wy = c[0] - x0, c[1] - y0
            out[py, px] = ((1 - wx) * (1 - wy) * tap(y0, x0) + wx * (1 - wy) * tap(y0, x0 + 1) +
                           (1 - wx) * wy * tap(y0 + 1, x0) + wx * wy * tap(y0 + 1, x0 + 1))
    return out


def pow2_scale(H, W, C, seed=0):
    """f32 [H][W][C] of signed powers of two in 1/4 .. 4"""
    rng = np.random.RandomState(500 + seed)
    return torch.from_numpy((2.0 ** rng.randint(-2, 3, size=(H, W, C)) * rng.choice([-1.0, 1.0], size=(H, W, C))).astype(np.float32))


# ===================================================================================================== comparison helpers
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _ordered(t):
    """the integer view mapped so that consecutive floats are consecutive integers (-0.0 and +0.0 coincide)"""
    i = t.contiguous().view(_INT_VIEW[t.dtype]).long()
    mask = 0x7FFFFFFF if t.dtype == torch.float32 else 0x7FFF
    return torch.where(i < 0, -(i & mask), i)


def _first(diff):
    idx = diff.nonzero()[0].tolist()
    return tuple(idx)


def assert_bits(got, want, what):
    """the integer views of the same dtype are equal; on failure: the first differing index ((roi, bin, channel) for a
    pooled tensor, (row, column, channel) for a map) and the count"""
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s vs %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    gi, wi = got.contiguous().view(_INT_VIEW[got.dtype]), want.contiguous().view(_INT_VIEW[want.dtype])
    diff = gi != wi
    n = int(diff.sum())
    if n:
        at = _first(diff)
        raise AssertionError("%s: %d of %d elements differ in their bits, first at %s: got %r, want %r" % (
            what, n, diff.numel(), at, float(got[at]), float(want[at])))


def assert_one_ulp(got, want, what, max_share):
    """every element within 1 ulp of its own dtype, and at most max_share of the elements different at all -> the share"""
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s vs %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    d = (_ordered(got) - _ordered(want)).abs()
    share = float((d > 0).double().mean())
    if int(d.max()) > 1:
        at = _first(d > 1)
        raise AssertionError("%s: %d elements are more than 1 ulp off, first at %s: got %r, want %r (%d ulp)" % (
            what, int((d > 1).sum()), at, float(got[at]), float(want[at]), int(d[at])))
    assert share <= max_share, "%s: %.3g of the elements differ by 1 ulp, more than %.3g (first at %s)" % (
        what, share, max_share, _first(d > 0))
    return share


def assert_per_pixel(got, want, tol, what):
    """|got - want| <= tol * max over channels of |want|, pixel by pixel ([H][W][C] tensors): a border pixel that is wrong by
    itself is not diluted by the rest of the map"""
    err = (got.double() - want.double()).abs().amax(-1)
    lim = tol * want.double().abs().amax(-1)
    bad = err > lim
    if bool(bad.any()):
        at = _first(bad)
        raise AssertionError("%s: %d pixels off, first at %s: |err| %.3g against %.3g" % (what, int(bad.sum()), at, float(err[at]), float(lim[at])))
    return float((err / lim.clamp(min=1e-30)).max())
