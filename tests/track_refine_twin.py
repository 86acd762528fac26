"""Test helper: a numpy twin of the track refinement as mega/pytorch_amd/tracks.py defines it, written as the definition's
loops: per video and track id the members in frame order, one interpolated box per gap frame (f32, one operation at a
time), then per box the window of the track's unsmoothed boxes within r frames, added in f64 in frame order.

Frames are tracks_twin's dicts {"box": [n,4] f32, "score": [n] f32, "label": [n] int} ("size" optional) plus "track": [n]
int (-1: in no track) and optionally "filled": [n] uint8; videos are (start, length) pairs.
"""
import numpy as np

import tracks_twin

f32 = np.float32


def to_boxlists(frames):
    """tracks_twin.to_boxlists plus the fields "track_ids" (int64) and, where a frame dict has it, "filled" (uint8)."""
    import torch
    out = tracks_twin.to_boxlists(frames)
    for b, f in zip(out, frames):
        b.add_field("track_ids", torch.from_numpy(np.asarray(f["track"], np.int64).copy()))
        if "filled" in f:
            b.add_field("filled", torch.from_numpy(np.asarray(f["filled"], np.uint8).copy()))
    return out


def from_boxlists(predictions):
    out = tracks_twin.from_boxlists(predictions)
    for f, p in zip(out, predictions):
        f["track"] = p.get_field("track_ids").cpu().numpy()
        if p.has_field("filled"):
            f["filled"] = p.get_field("filled").cpu().numpy()
    return out


def refine(frames, videos, fill=True, smooth=0, fill_scale=1.0):
    """-> (the refined frames: dicts with "box", "score", "label", "track", "filled" (and "size" where the input has it),
    the input boxes first, then the frame's filled boxes by ascending track id; {"tracks": K, "filled": n_new})."""
    scale = f32(fill_scale)
    box = [np.asarray(f["box"], f32).reshape(-1, 4).copy() for f in frames]
    added = [[] for _ in frames]                      # per frame: (box, score, label, id) of its filled boxes
    n_tracks = 0
    for s0, n in videos:
        ids = set()
        for f in frames[s0:s0 + n]:
            ids.update(int(i) for i in np.asarray(f["track"]) if i >= 0)
        for tid in sorted(ids):
            n_tracks += 1
            members = [(t, i) for t in range(s0, s0 + n) for i, v in enumerate(np.asarray(frames[t]["track"])) if v == tid]
            label = int(np.asarray(frames[members[0][0]]["label"])[members[0][1]])
            seq = []                                  # the track's unsmoothed boxes by frame: (frame, box, index or None, score)
            for m, (t, i) in enumerate(members):
                b = np.asarray(frames[t]["box"], f32).reshape(-1, 4)[i]
                if m and fill:
                    ta, ia = members[m - 1]
                    a = np.asarray(frames[ta]["box"], f32).reshape(-1, 4)[ia]
                    sa = np.asarray(frames[ta]["score"], f32)[ia] + f32(0)      # (-0.0 counts as +0.0)
                    sb = np.asarray(frames[t]["score"], f32)[i] + f32(0)
                    for f in range(ta + 1, t):
                        w = f32(f - ta) / f32(t - ta)
                        c = np.zeros(4, f32)
                        for k in range(4):
                            d = f32(b[k] - a[k])
                            p = f32(d * w)
                            c[k] = f32(a[k] + p)
                        seq.append((f, c, None, f32(min(sa, sb) * scale)))
                seq.append((t, b.copy(), i, None))
            for t, c, i, sc in seq:
                new = c
                if smooth > 0:
                    win = [c2 for t2, c2, _, _ in seq if abs(t2 - t) <= smooth]
                    new = np.zeros(4, f32)
                    for k in range(4):
                        acc = np.float64(win[0][k])
                        for c2 in win[1:]:
                            acc = acc + np.float64(c2[k])
                        new[k] = f32(acc / np.float64(len(win)))
                if i is not None:
                    box[t][i] = new
                else:
                    added[t].append((new, sc, label, tid))
    out = []
    for f, b, add in zip(frames, box, added):
        n = len(b)
        old = np.asarray(f["filled"], np.uint8) if "filled" in f else np.zeros(n, np.uint8)
        g = {"box": np.concatenate([b] + [a[0][None] for a in add]).astype(f32).reshape(-1, 4),
             "score": np.concatenate([np.asarray(f["score"], f32), np.asarray([a[1] for a in add], f32)]),
             "label": np.concatenate([np.asarray(f["label"], np.int64), np.asarray([a[2] for a in add], np.int64)]),
             "track": np.concatenate([np.asarray(f["track"], np.int64), np.asarray([a[3] for a in add], np.int64)]),
             "filled": np.concatenate([old, np.ones(len(add), np.uint8)])}
        if "size" in f:
            g["size"] = f["size"]
        out.append(g)
    return out, {"tracks": n_tracks, "filled": sum(len(a) for a in added)}
