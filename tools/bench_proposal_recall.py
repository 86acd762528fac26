"""Times the VID proposal recall (mega.pytorch_amd.vid_eval.evaluate_proposals) at ImageNet VID validation size: 176,126
frames x 300 proposals against seeded GT of 1-6 boxes per frame.  Prints one JSON line:

  kernel_ms      the matching kernel alone (device events around ops.proposal_recall_match on resident inputs, the
                 median of --repeats launches after a warm-up), for limit 300 and for the four-limit table launch
  end_to_end_s   evaluate_proposals on the list[BoxList]: host concatenation and checks, one host-to-device copy, the
                 device sort, the kernel, the threshold counts and the copy back (host clock, ends in a synchronise)

  python tools/bench_proposal_recall.py [--frames 176126] [--proposals 300] [--repeats 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(frames, proposals, seed):
    """-> (list[BoxList] with "objectness" in a 1000 x 600 frame, VIDGroundTruth in 1280 x 720): per frame 1-6 GT boxes,
    60 % of the proposals jittered around them, the rest clutter; objectness descending, as an RPN hands them over."""
    from mega.pytorch_amd import vid_eval
    from mega.pytorch_amd.structures import BoxList
    rng = np.random.default_rng(seed)
    W, H, pw, ph = 1280, 720, 1000, 600
    g = rng.integers(1, 7, frames)
    off = np.concatenate([[0], np.cumsum(g)]).astype(np.int64)
    G = int(off[-1])
    x1, y1 = rng.uniform(0, W * 0.7, G), rng.uniform(0, H * 0.7, G)
    gb = np.round(np.stack([x1, y1, np.minimum(x1 + rng.uniform(16, W * 0.3, G), W - 1),
                            np.minimum(y1 + rng.uniform(16, H * 0.3, G), H - 1)], 1)).astype(np.float32)
    gt = vid_eval.VIDGroundTruth.__new__(vid_eval.VIDGroundTruth)
    gt.image_set_index = None
    gt._set(gb, np.ones(G, np.int64), off, np.full(frames, H), np.full(frames, W))
    pick = off[:-1, None] + (rng.integers(0, 1 << 30, (frames, proposals)) % g[:, None])
    near = gb[pick] + rng.normal(0, 12, (frames, proposals, 4)).astype(np.float32)
    cx, cy = rng.uniform(0, W, (frames, proposals)), rng.uniform(0, H, (frames, proposals))
    w, h = rng.uniform(8, W / 3, (frames, proposals)), rng.uniform(8, H / 3, (frames, proposals))
    clutter = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)
    box = np.where((rng.random((frames, proposals)) < 0.6)[..., None], near, clutter)
    box = np.clip(box * np.float32([pw / W, ph / H, pw / W, ph / H]), 0, np.float32([pw - 1, ph - 1, pw - 1, ph - 1]))
    box = torch.from_numpy(np.ascontiguousarray(box, np.float32))
    obj = torch.from_numpy(-np.sort(-rng.random((frames, proposals)).astype(np.float32), axis=1))
    preds = []
    for f in range(frames):
        b = BoxList(box[f], (pw, ph))
        b.add_field("objectness", obj[f])
        preds.append(b)
    return preds, gt


def kernel_ms(args, repeats):
    from mega.pytorch_amd import ops
    ops.proposal_recall_match(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.proposal_recall_match(*args)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--proposals", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("bench_proposal_recall needs a HIP device (no CPU path)")
    from mega.pytorch_amd import vid_eval
    dev = torch.device(a.device)
    preds, gt = make(a.frames, a.proposals, a.seed)
    out = {"bench": "proposal_recall", "frames": a.frames, "proposals_per_frame": a.proposals, "gt_boxes": int(gt.off[-1])}
    with torch.cuda.device(dev):
        one = vid_eval.proposal_inputs(preds, gt, [300], dev)
        out["kernel_ms"] = round(kernel_ms(one, a.repeats), 4)
        four = vid_eval.proposal_inputs(preds, gt, list(vid_eval.PROPOSAL_LIMITS), dev)
        out["kernel_table_ms"] = round(kernel_ms(four, a.repeats), 4)
        del one, four
        vid_eval.evaluate_proposals(preds[:64], vid_eval.VIDGroundTruth.from_annotations(
            [{"boxes": gt.boxes[gt.off[i]:gt.off[i + 1]], "labels": gt.labels[gt.off[i]:gt.off[i + 1]],
              "im_info": (int(gt.height[i]), int(gt.width[i]))} for i in range(64)]), device=dev)      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = vid_eval.evaluate_proposals(preds, gt, device=dev)
        torch.cuda.synchronize()
        out["end_to_end_s"] = round(time.perf_counter() - t0, 4)
        t0 = time.perf_counter()
        tab = vid_eval.evaluate_proposals(preds, gt, limits=vid_eval.PROPOSAL_LIMITS, device=dev)
        torch.cuda.synchronize()
        out["end_to_end_table_s"] = round(time.perf_counter() - t0, 4)
    out["recall"] = round(float(res["recall"]), 6)
    out["ar"] = [round(float(v), 6) for v in tab["ar"]]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
