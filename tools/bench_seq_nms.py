"""Times Seq-NMS (mega.pytorch_amd.seq_nms) on a seeded synthetic set the size of ImageNet VID val: 555 videos, 176,126
frames, 300 detections per frame over 30 classes -- temporally coherent jittered tracks with near-duplicates and per-frame
score dips, and clutter with scores mostly near 0.001.  Video lengths are long-tailed (the longest >= 2,000 frames).

  python tools/bench_seq_nms.py [--videos 555] [--frames 176126] [--dets 300] [--warmup 1] [--repeats 3]
      wall time list[BoxList] -> list[BoxList] (host packing and checks, one copy in, sorts, the kernel, one copy back,
      the per-frame split): median of the repeats after the warm-up; plus the task count, the largest box count and
      iteration count of a task and the DP frame steps recomputed (one extra, untimed run).  One JSON line.
      Kernel times: run it under  rocprofv3 --kernel-trace --stats -- python tools/bench_seq_nms.py
  python tools/bench_seq_nms.py --twin-cpu --subset 3
      CPU only: the numpy twin (tests/seq_nms_twin.py) on the first --subset videos of the same set; reports the measured
      time and a LINEAR EXTRAPOLATION by frame count to the full set.
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def video_lengths(videos, frames, rng, longest=2400):
    """Long-tailed lengths summing to `frames`, the longest `longest` frames."""
    raw = rng.lognormal(0.0, 0.9, videos)
    raw[int(np.argmax(raw))] = 0.0
    rest = frames - longest
    lens = np.maximum(1, np.floor(raw / raw.sum() * rest)).astype(np.int64)
    lens[int(np.argmax(raw == 0.0))] = longest
    d = frames - int(lens.sum())
    order = np.argsort(-lens)
    i = 1
    while d != 0:       # spread the rounding remainder over the longer videos (not the longest)
        k = order[i % (videos - 1) + 1 if videos > 1 else 0]
        step = 1 if d > 0 else (-1 if lens[k] > 1 else 0)
        lens[k] += step
        d -= step
        i += 1
    return lens


def make_set(videos=555, frames=176126, dets=300, classes=30, seed=0, lengths=None):
    """-> {"box" [N,4] f32, "score" [N] f32, "label" [N] i64, "videos" [(start, length)], "dets"}, N = frames * dets; and
    the tracks the detections were jittered around as ground truth: "gt_box" [G,4] f32 (rounded, clipped), "gt_label" [G]
    i64, "gt_track" [G] i64 (the track's number within its video), "gt_off" [F+1] i64 (frame f's GT boxes)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lengths, np.int64) if lengths is not None else video_lengths(videos, frames, rng)
    F = int(lens.sum())
    box = np.empty((F, dets, 4), np.float32)
    score = np.empty((F, dets), np.float32)
    label = np.empty((F, dets), np.int64)
    W, H, DUP = 640.0, 480.0, 3
    f0 = 0
    vids = []
    gt_box, gt_label, gt_track, gt_count = [], [], [], np.zeros(F, np.int64)
    for L in lens.tolist():
        vids.append((f0, L))
        K = int(rng.integers(1, 7))                          # tracks in this video
        t = np.arange(L)[None, :, None]
        wh = rng.uniform([30, 30], [W * 0.4, H * 0.4], (K, 2))
        p0 = rng.uniform([0, 0], [W * 0.6, H * 0.6], (K, 2))
        v = rng.normal(0, 1.0, (K, 2))
        xy = p0[:, None, :] + v[:, None, :] * t + rng.normal(0, 1.0, (K, L, 2))
        tb = np.concatenate([xy, xy + wh[:, None, :]], 2)    # [K, L, 4]
        t_start = rng.integers(0, max(L // 2, 1), K)
        t_len = rng.integers(np.maximum(L // 4, 1), L + 1, K)
        active = (np.arange(L)[None, :] >= t_start[:, None]) & (np.arange(L)[None, :] < (t_start + t_len)[:, None])
        tcls = rng.integers(1, classes + 1, K)
        tsc = rng.uniform(0.5, 0.98, (K, L))
        tsc = np.where(rng.random((K, L)) < 0.15, tsc * rng.uniform(0.02, 0.3, (K, L)), tsc)   # per-frame dips
        # clutter everywhere, then the track slots on top: slot k * (1 + DUP) main box, the next DUP near-duplicates
        c_xy = rng.uniform([0, 0], [W, H], (L, dets, 2))
        c_wh = rng.uniform(8, 200, (L, dets, 2))
        vb = np.concatenate([c_xy - c_wh / 2, c_xy + c_wh / 2], 2)
        vs = np.minimum(rng.exponential(0.002, (L, dets)) + 0.0005, 0.4)
        vl = rng.integers(1, classes + 1, (L, dets))
        for k in range(K):
            for d in range(1 + DUP):
                slot = k * (1 + DUP) + d
                if slot >= dets:
                    break
                a = active[k]
                jit = rng.normal(0, 2.0 if d == 0 else 8.0, (L, 4))
                vb[a, slot] = tb[k, a] + jit[a]
                vs[a, slot] = tsc[k, a] if d == 0 else tsc[k, a] * rng.uniform(0.3, 0.9, int(a.sum()))
                vl[a, slot] = tcls[k]
        vb = np.sort(vb.reshape(L, dets, 2, 2), axis=2).reshape(L, dets, 4)
        box[f0:f0 + L] = np.clip(vb, 0, [W - 1, H - 1, W - 1, H - 1])
        score[f0:f0 + L] = vs
        label[f0:f0 + L] = vl
        tt, kk = np.nonzero(active.T)                        # (frame, track) of every GT box, frame-major
        gt_box.append(np.round(np.clip(tb[kk, tt], 0, [W - 1, H - 1, W - 1, H - 1])).astype(np.float32))
        gt_label.append(tcls[kk].astype(np.int64))
        gt_track.append(kk.astype(np.int64))
        gt_count[f0:f0 + L] = active.sum(0)
        f0 += L
    gt_off = np.zeros(F + 1, np.int64)
    gt_off[1:] = np.cumsum(gt_count)
    return {"box": box.reshape(-1, 4), "score": score.reshape(-1), "label": label.reshape(-1), "videos": vids,
            "dets": dets, "gt_box": np.concatenate(gt_box).reshape(-1, 4), "gt_label": np.concatenate(gt_label),
            "gt_track": np.concatenate(gt_track), "gt_off": gt_off}


def to_boxlists(s, lo=0, hi=None):
    """BoxLists of frames lo .. hi (views into the flat arrays)."""
    import torch
    from mega.pytorch_amd.structures import BoxList
    D = s["dets"]
    hi = len(s["score"]) // D if hi is None else hi
    boxes = torch.from_numpy(s["box"][lo * D:hi * D]).split(D)
    scores = torch.from_numpy(s["score"][lo * D:hi * D]).split(D)
    labels = torch.from_numpy(s["label"][lo * D:hi * D]).split(D)
    out = []
    for b, sc, lb in zip(boxes, scores, labels):
        x = BoxList(b, (640, 480))
        x.add_field("scores", sc)
        x.add_field("labels", lb)
        out.append(x)
    return out


def to_frames(s, lo, hi):
    D = s["dets"]
    return [{"box": s["box"][f * D:(f + 1) * D], "score": s["score"][f * D:(f + 1) * D],
             "label": s["label"][f * D:(f + 1) * D]} for f in range(lo, hi)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--videos", type=int, default=555)
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rescore", choices=("avg", "max"), default="avg")
    ap.add_argument("--twin-cpu", action="store_true", help="time the numpy twin on --subset videos (CPU only)")
    ap.add_argument("--subset", type=int, default=3)
    a = ap.parse_args(argv)
    s = make_set(a.videos, a.frames, a.dets, seed=a.seed)
    F = len(s["score"]) // a.dets
    lens = [n for _, n in s["videos"]]
    base = {"videos": len(s["videos"]), "frames": F, "boxes": len(s["score"]), "longest_video": max(lens),
            "rescore": a.rescore, "host": platform.node()}
    if a.twin_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import seq_nms_twin
        sub = s["videos"][:a.subset]
        hi = sub[-1][0] + sub[-1][1]
        frames = to_frames(s, 0, hi)
        t0 = time.perf_counter()
        _, _, iters = seq_nms_twin.seq_nms(frames, sub, rescore=a.rescore)
        dt = time.perf_counter() - t0
        print(json.dumps(dict(base, metric="seq_nms_twin_cpu_s", subset_videos=len(sub), subset_frames=hi,
                              measured_s=round(dt, 3), max_task_iterations=max(iters.values()),
                              extrapolated_full_s=round(dt * F / max(hi, 1), 1),
                              note="linear extrapolation by frame count from the measured subset")))
        return 0
    import torch
    from mega.pytorch_amd import seq_nms
    preds = to_boxlists(s)
    dev = "cuda:0"
    times = []
    for r in range(a.warmup + a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = seq_nms.seq_nms(preds, s["videos"], rescore=a.rescore, device=dev)
        torch.cuda.synchronize()
        if r >= a.warmup:
            times.append(time.perf_counter() - t0)
    kept = sum(len(p) for p in out)
    st = seq_nms.run(preds, s["videos"], rescore=a.rescore, device=dev, with_stats=True)
    tasks, stats = st["tasks"], st["stats"]
    task_boxes = None
    if len(tasks):
        pk = st["packed"]
        task_boxes = int(max(np.count_nonzero((pk["labels"] == tasks[0, 0]) &
                                              (np.repeat(np.arange(F), pk["counts"]) >= tasks[0, 1]) &
                                              (np.repeat(np.arange(F), pk["counts"]) < tasks[0, 1] + tasks[0, 2])), 0))
    print(json.dumps(dict(base, metric="seq_nms_wall_s", median_s=round(float(np.median(times)), 4),
                          times_s=[round(t, 4) for t in times], warmup=a.warmup, kept=kept, tasks=int(len(tasks)),
                          max_task_boxes=task_boxes, max_task_iterations=int(stats[:, 0].max()) if len(stats) else 0,
                          total_iterations=int(stats[:, 0].sum()), dp_frame_steps=int(stats[:, 1].sum()),
                          full_dp_frame_steps_per_iteration=int(tasks[:, 2].sum()) if len(tasks) else 0)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
