"""Evidence for TEST.SOFT_NMS / TEST.BBOX_VOTE: prints ONE JSON line with the device time per frame of the
final filter on a workload-sized synthetic chunk -- 16 frames, 31 classes, 300 rows per view, K = 1 and K = 4 views, ~30 %
of the candidates above the threshold, boxes clustered around 6 objects per (frame, class) so that the chains of
dependent soft-NMS steps are as long as crowded frames make them:
  bbox_aug_merge   the yardstick: the greedy-NMS merge (ops.bbox_aug_merge)
  linear / gaussian / hard_vote / gaussian_vote   ops.soft_merge in these modes
  steps            the longest (frame, class) problem's soft-NMS step count (= its kept rows), linear and gaussian
Timing: HIP events around --inner back-to-back calls, --reps windows per leg, the legs alternating inside every
repetition, median and min-max spread reported; every leg is warmed up first.  No GPU, no number: this tool has no
fallback.
usage: python tools/bench_soft_nms.py [--reps 15] [--inner 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, C1, R = 16, 30, 300
SIZES = [(1000, 600), (1000, 600), (833, 500), (833, 500)]
FLIPS = [False, True, False, True]


def candidates(K, dev, seed=0, centres=6, p_live=0.3):
    """-> cboxes [K,F,C1,R,4] (each view's boxes in its own image), cscores [K,F,C1,R] (-1 = dead), seeded"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    w0, h0 = SIZES[0]
    ctr = torch.rand((F, C1, centres, 2), generator=g) * torch.tensor([w0 * 0.7, h0 * 0.7]) + torch.tensor([w0 * 0.15, h0 * 0.15])
    half = torch.rand((F, C1, centres, 2), generator=g) * torch.tensor([w0 * 0.10, h0 * 0.10]) + torch.tensor([w0 * 0.04, h0 * 0.04])
    cbs, css = [], []
    for k in range(K):
        which = torch.randint(0, centres, (F, C1, R), generator=g)
        idx = which[..., None].expand(F, C1, R, 2)
        hf = torch.gather(half, 2, idx)
        c = torch.gather(ctr, 2, idx) + torch.randn((F, C1, R, 2), generator=g) * hf * 0.18
        hf = hf * (1 + torch.randn((F, C1, R, 2), generator=g) * 0.10)
        b = torch.cat([c - hf, c + hf], -1)
        w, h = SIZES[k]
        b = b * torch.tensor([w / w0, h / h0, w / w0, h / h0])
        if FLIPS[k]:
            b = torch.stack([w - b[..., 2] - 1, b[..., 1], w - b[..., 0] - 1, b[..., 3]], -1)
        b = torch.minimum(b.clamp(min=0), torch.tensor([w - 1., h - 1., w - 1., h - 1.]))
        s = torch.rand((F, C1, R), generator=g) * 0.98 + 0.01
        s = torch.where(torch.rand((F, C1, R), generator=g) < p_live, s, torch.full_like(s, -1.0))
        cbs.append(b)
        css.append(s)
    return torch.stack(cbs).float().to(dev).contiguous(), torch.stack(css).float().to(dev).contiguous()


def legs(ops, cb, cs, K):
    sizes, flips = SIZES[:K], FLIPS[:K]

    def soft(**kw):
        return lambda max_det=300: ops.soft_merge(cb, cs, sizes, flips, 0.001, 0.5, max_det, True, **kw)
    return [("bbox_aug_merge", lambda max_det=300: ops.bbox_aug_merge(cb, cs, sizes, flips, 0.001, 0.5, max_det, True)),
            ("linear", soft(soft_method="linear")),
            ("gaussian", soft(soft_method="gaussian", sigma=0.5)),
            ("hard_vote", soft(vote=True, vote_thresh=0.8)),
            ("gaussian_vote", soft(soft_method="gaussian", sigma=0.5, vote=True, vote_thresh=0.8))]


def longest_chain(fn):
    """the largest kept count of a (frame, class) problem without the detections-per-image cut = its step count"""
    _, _, ol, oc = fn(max_det=0)
    best = 0
    for f, n in enumerate(oc.tolist()):
        if n:
            best = max(best, int(torch.bincount(ol[f, :n]).max()))
    return best


def measure(dev, K, reps, inner):
    from mega.pytorch_amd import ops
    cb, cs = candidates(K, dev)
    ls = legs(ops, cb, cs, K)
    for _, fn in ls:
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    ts = {name: [] for name, _ in ls}
    for _ in range(reps):
        for name, fn in ls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) / inner)
    out = {"live_rows_per_class": round(float((cs >= 0).sum()) / (F * C1), 1)}
    for name, v in ts.items():
        v.sort()
        out[name] = {"us_per_frame": round(1000 * v[len(v) // 2] / F, 2), "min": round(1000 * v[0] / F, 2),
                     "max": round(1000 * v[-1] / F, 2)}
    out["steps"] = {"linear": longest_chain(ls[1][1]), "gaussian": longest_chain(ls[2][1])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_nms: no HIP device (there is no CPU fallback, and no CPU number)")
    dev = torch.device("cuda:0")
    res = {"frames": F, "classes": C1 + 1, "rows": R, "reps": a.reps, "calls_per_window": a.inner,
           "unit": "device us per frame (median of the windows; min, max)"}
    for K in (1, 4):
        res["K%d" % K] = measure(dev, K, a.reps, a.inner)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
