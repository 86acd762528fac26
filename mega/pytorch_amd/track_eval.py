"""Tubelet AP: linked tracks scored against the ground-truth tracks of ImageNet VID -- the tubelet-level AP of the ILSVRC
"object detection / tracking from video" task.  A predicted tubelet is right when it covers one GT track well enough in
time; coverage is measured at the thresholds 0.25, 0.5 and 0.75.

The reference has no counterpart; this docstring defines it, and the kernel (csrc/track_eval.hip) and the test twin
(tests/track_eval_twin.py) implement this definition.

Inputs.  predictions: a list[BoxList] in dataset order with "scores" (f32, >= 0 as for tracks.link), "labels" and
"track_ids" (int64, -1 = in no track): what tracks.link returns or predictions_tracks.pth holds.  videos: as for
tracks.link.  groundtruth: a vid_eval.VIDTrackGroundTruth of the same frames (a GT that also carries a track id per box).

Tubelet.  All boxes of one video with the same track_ids >= 0.  Its label is its boxes' label.  Its score is an f64: with
tubelet_score="mean" (the default) the sum of the members' f32 scores, added in f64 in frame order, divided by the count;
with "max" the largest member score.

GT track.  All GT boxes of one video with the same <trackid>.  The GT tracks of a video are numbered 0, 1, ... by
ascending track id.

Host checks (ValueError with the prefix "track_eval:", before any device work): track_ids < -1; two boxes of one tubelet,
or of one GT track, in the same frame; a tubelet or GT track with more than one label; a NaN (or negative) score; a non-
finite box; a negative label; predictions and ground truth of different lengths; a missing "track_ids" field.

Frame hit.  A tubelet p and a GT track g of the same video and label both have a box in frame f, and the box IoU is
>= 0.5f.  The box IoU is exactly the detection AP's, with the same >=: the prediction is rescaled to the annotation's
frame size by one f32 multiply per coordinate; +1 is added to x2 / y2 of both boxes; then box_math.h's box_iou1 (the +1
convention in f32, no FMA contraction).  That is csrc/box_math.h's vid_iou, the one function vid_eval.hip calls too.  A
NaN IoU is no hit.

Pair counts, all integers:  both(p, g) = frames where both have a box;  hits(p, g) = frame hits;
union(p, g) = len(p) + len(g) - both(p, g).

Temporal IoU.  tIoU = hits / union, never formed as a float:  tIoU >= num / den  means  hits * den >= num * union  in
64-bit integers;  tIoU(a) > tIoU(b)  means  hits_a * union_b > hits_b * union_a.

Thresholds.  Rational pairs, by default ((1, 4), (1, 2), (3, 4)); each (num, den) must satisfy 0 < num <= den <= 1024 (at
most 8 of them).

Matching.  Per threshold, independently per (video, label): the tubelets go in descending score, equal scores by
ascending track id.  Each takes one GT track among those that are not yet taken, have hits > 0 and a tIoU that reaches
the threshold: the one with the largest tIoU, on an equal tIoU (1/2 against 2/4) the lowest GT track number.  If it takes
one it is a true positive and that GT track is taken; otherwise it is a false positive.  There is no ignore class.

AP.  Per label and threshold over the label's tubelets of the whole dataset, in descending score, equal scores by
ascending (video, track id).  n_pos is the label's number of GT tracks.  The formula is the detection AP's:
ops.vid_eval_ap with pred_ignore = 0; a label without GT tracks gives what that kernel gives for n_pos = 0 (NaN).

Result.  ap [R, C] f64 (C = the largest label seen + 1);  map [R], the nanmean over the foreground labels 1 .. C-1;  mean,
the mean of the R maps;  and a table with one row per GT track: video, GT track number, label, length and, for the (1, 2)
threshold (the first threshold if none equals 1/2), the id of the tubelet that took the track (-1 for none) with the
pair's hits and union (0 for none).

Text (result_tubelets.txt): one "tubelet AP | tIoU>=0.25 = x.xxxx" line per threshold, a mean line, and "Category AP:"
lines of that same threshold in vid_eval.format_result's layout.

There is no CPU path: one workgroup per (video, label) task that has a tubelet and a GT track counts the pairs' both /
hits and matches (csrc/track_eval.hip); tubelet scores, ranks and the per-label order are segment operations on the
device; the AP is vid_eval's kernel.  A (video, label) holds at most 4096 GT tracks.
"""
import warnings

import numpy as np
import torch

from . import flat, vid_eval

THRESHOLDS = ((1, 4), (1, 2), (3, 4))
SCORE_MODES = ("mean", "max")
MAX_THRESHOLDS = 8
MAX_GT_TRACKS = 4096        # per (video, label): the kernel keeps 64 taken flags per lane
LDS_PAIRS = 4096            # csrc/track_eval.hip TE_LDS_PAIRS: a task's P x G tables beyond this live in the workspace
TUBELET_DTYPE = np.dtype([("video", np.int64), ("id", np.int64), ("label", np.int64), ("count", np.int64),
                          ("score", np.float64)])
GT_TABLE_DTYPE = np.dtype([("video", np.int64), ("gt", np.int64), ("label", np.int64), ("count", np.int64),
                           ("tubelet", np.int64), ("hits", np.int64), ("union", np.int64)])


def check_params(thresholds=THRESHOLDS, tubelet_score="mean"):
    """-> the thresholds as a tuple of (num, den) int pairs; ValueError for a bad value."""
    if tubelet_score not in SCORE_MODES:
        raise ValueError("track_eval: tubelet_score must be one of %s, got %r" % (SCORE_MODES, tubelet_score))
    try:
        thr = tuple((nd[0], nd[1]) for nd in thresholds)
        assert all(len(nd) == 2 for nd in thresholds)
    except Exception:
        raise ValueError("track_eval: thresholds must be (num, den) pairs, got %r" % (thresholds,))
    if not 0 < len(thr) <= MAX_THRESHOLDS:
        raise ValueError("track_eval: 1 to %d thresholds, got %d" % (MAX_THRESHOLDS, len(thr)))
    for n, d in thr:
        for v in (n, d):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("track_eval: a threshold is a pair of ints, got %r" % ((n, d),))
        if not 0 < n <= d <= 1024:
            raise ValueError("track_eval: a threshold (num, den) needs 0 < num <= den <= 1024, got %r" % ((n, d),))
    return tuple((int(n), int(d)) for n, d in thr)


def table_threshold(thresholds):
    """The index of the threshold the GT table and the per-category lines use: the first equal to 1/2, else 0."""
    for i, (n, d) in enumerate(thresholds):
        if 2 * n == d:
            return i
    return 0


def _segment_checks(key, frame, label, what):
    """key / frame / label of every box (frame ascending within the array): ValueError if two boxes of one key share a
    frame or differ in label."""
    if key.size < 2:
        return
    o = np.argsort(key, kind="stable")
    k, f, l = key[o], frame[o], label[o]
    same = k[1:] == k[:-1]
    if (same & (f[1:] == f[:-1])).any():
        raise ValueError("track_eval: two boxes of one %s in the same frame" % what)
    if (same & (l[1:] != l[:-1])).any():
        raise ValueError("track_eval: a %s with more than one label" % what)


def _pack(predictions, groundtruth, videos):
    """The host checks and the flat host arrays of both sides."""
    F = len(predictions)
    if not hasattr(groundtruth, "track_ids"):
        raise ValueError("track_eval: the ground truth carries no track ids (use vid_eval.VIDTrackGroundTruth)")
    if len(groundtruth) != F:
        raise ValueError("track_eval: %d predictions, %d GT frames" % (F, len(groundtruth)))
    if F == 0:
        raise ValueError("track_eval: no predictions")
    for p in predictions:
        if not p.has_field("track_ids"):
            raise ValueError("track_eval: a prediction has no field \"track_ids\" (fields: %r); link the detections with "
                             "tracks.link first" % (sorted(p.fields()),))
    pk = flat.pack(predictions, videos, "track_eval")
    N = pk["N"]
    tid = torch.cat([p.get_field("track_ids").reshape(-1).to("cpu", torch.int64) for p in predictions]).numpy() if N \
        else np.zeros(0, np.int64)
    if N and tid.min() < -1:
        raise ValueError("track_eval: a track id below -1")
    if N and tid.max() >= 0x7fffffff:
        raise ValueError("track_eval: a track id does not fit 31 bits")
    gl, gb, gt_tid = groundtruth.labels, groundtruth.boxes, np.asarray(groundtruth.track_ids, np.int64)
    if not np.isfinite(gb).all():
        raise ValueError("track_eval: a GT box is not finite")
    if gl.size and gl.min() < 0:
        raise ValueError("track_eval: negative class label")
    if gt_tid.shape != gl.shape:
        raise ValueError("track_eval: %d GT boxes, %d GT track ids" % (gl.size, gt_tid.size))
    C = max(pk["C"], int(gl.max()) + 1 if gl.size else 0)
    if C <= 0:
        raise ValueError("track_eval: no class occurs in the predictions or the GT")
    if C * F >= 0x7fffffff:
        raise ValueError("track_eval: %d classes x %d frames: too many" % (C, F))
    vs, vl = pk["video_start"], pk["video_len"]
    V = len(vs)
    vid_of_frame = np.repeat(np.arange(V, dtype=np.int64), vl)
    # tubelets: the boxes with an id
    fid = np.repeat(np.arange(F, dtype=np.int64), pk["counts"])
    m = tid >= 0
    mfid, mtid, mlab = fid[m], tid[m], pk["labels"][m]
    K = int(mtid.max()) + 1 if mtid.size else 1
    _segment_checks(vid_of_frame[mfid] * K + mtid, mfid, mlab, "tubelet")
    # GT tracks, sorted by (video, track id): number = position within the video
    gfid = np.repeat(np.arange(F, dtype=np.int64), np.diff(groundtruth.off))
    gvid = vid_of_frame[gfid]
    if gt_tid.size:
        lo = int(gt_tid.min())
        if int(gt_tid.max()) - lo >= 0x7fffffff:
            raise ValueError("track_eval: the GT track ids span more than 31 bits")
        gkey = gvid * (int(gt_tid.max()) - lo + 1) + (gt_tid - lo)
    else:
        gkey = np.zeros(0, np.int64)
    _segment_checks(gkey, gfid, gl, "GT track")
    uniq, first, inv, glen = np.unique(gkey, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    J = len(uniq)
    j_vid, j_lab = gvid[first], gl[first]
    vfirst = np.zeros(V + 1, np.int64)
    vfirst[1:] = np.cumsum(np.bincount(j_vid, minlength=V))
    j_num = np.arange(J, dtype=np.int64) - vfirst[j_vid]
    # GT slots: by (video, label), within by number -- a task's GT tracks are g0 .. g0 + G
    jorder = np.lexsort((j_num, j_lab, j_vid))
    slot_of_j = np.empty(J, np.int64)
    slot_of_j[jorder] = np.arange(J)
    grp = j_vid * C + j_lab
    g_cnt = np.bincount(grp, minlength=V * C).astype(np.int64)
    if J and g_cnt.max() > MAX_GT_TRACKS:
        raise ValueError("track_eval: a (video, label) holds %d GT tracks (at most %d)" % (g_cnt.max(), MAX_GT_TRACKS))
    g_start = np.zeros(V * C + 1, np.int64)
    g_start[1:] = np.cumsum(g_cnt)
    # GT boxes class-major then frame; each with its track's index within its (video, label)
    bkey = gl * F + gfid
    border = np.argsort(bkey, kind="stable")
    gt_seg_off = np.zeros(C * F + 1, np.int64)
    gt_seg_off[1:] = np.cumsum(np.bincount(bkey, minlength=C * F))
    local = slot_of_j[inv] - g_start[grp[inv]]
    gt = {"J": J, "box": gb[border], "track": local[border].astype(np.int32), "seg_off": gt_seg_off,
          "len": glen[jorder].astype(np.int32), "g_cnt": g_cnt, "g_start": g_start[:-1].copy(),
          "slot_video": j_vid[jorder], "slot_num": j_num[jorder], "slot_label": j_lab[jorder],
          "n_pos": np.bincount(j_lab, minlength=C).astype(np.int32)}
    members = {"F": F, "N": int(m.sum()), "C": C, "counts": np.bincount(mfid, minlength=F).astype(np.int64),
               "boxes": pk["boxes"][m], "scores": pk["scores"][m], "labels": mlab, "video_start": vs, "video_len": vl}
    return members, mtid, K, gt, V


def run(predictions, groundtruth, videos, thresholds=THRESHOLDS, tubelet_score="mean", device="cuda", pairs=True,
        return_workspace=False):
    """The evaluation as host arrays:
      "tubelets"    [U] TUBELET_DTYPE, by (video, track id): video, id, label, box count, score
      "match"       [R, U] u8 and "matched_gt" [R, U] i64: per threshold, whether the tubelet is a true positive and the
                    number (within the video) of the GT track it took, -1 for none
      "n_pos"       [C] i64, "ap" [R, C] f64
      "gt_table"    [J] GT_TABLE_DTYPE, by (video, label, GT track number)
      "pairs"       (with pairs=True) {(video, label): {"tubelets": track ids in rank order, "gt": GT track numbers,
                    "hits": [P, G], "both": [P, G]}} for every (video, label) with a tubelet and a GT track
      "ws_pairs"    the pairs whose tables lived in the kernel's workspace, not in LDS; with return_workspace also
                    "workspace": the workspace's (hits, both) arrays after the launch, preset to -1."""
    thr = check_params(thresholds, tubelet_score)
    R = len(thr)
    dev = torch.device(device)
    flat.require_hip(dev, "track_eval", device)
    mem, mtid, K, gt, V = _pack(predictions, groundtruth, videos)
    F, M, C, J = mem["F"], mem["N"], mem["C"], gt["J"]
    from . import ops
    out = {"thresholds": thr, "n_pos": gt["n_pos"].astype(np.int64), "ws_pairs": 0}
    with torch.cuda.device(dev):
        g = flat.upload([("box", gt["box"]), ("track", gt["track"]), ("seg_off", gt["seg_off"]), ("len", gt["len"]),
                         ("g_cnt", gt["g_cnt"]), ("g_start", gt["g_start"]), ("n_pos", gt["n_pos"]),
                         ("ratio", vid_eval._resize_ratios(predictions, groundtruth)), ("tid", mtid)], dev)
        n_pos = g["n_pos"][None, :].expand(R, C).contiguous()
        if M == 0:
            U = 0
            z64 = torch.zeros(0, dtype=torch.int64, device=dev)
            u_vid = u_tid = u_lab = u_len = z64
            u_score = torch.zeros(0, dtype=torch.float64, device=dev)
            match = torch.zeros((R, 0), dtype=torch.uint8, device=dev)
            mgt = torch.zeros((R, 0), dtype=torch.int32, device=dev)
            T = 0
        else:
            v = flat.video_tasks(mem, dev, by_score=False)
            t, fid, order = v["t"], v["fid"], v["order"]
            vid_of_frame = flat.frame_ids(t["vl"], dev, F)
            # tubelets: the distinct (video, track id), in that order
            uniq, inv, u_len = torch.unique(vid_of_frame[fid] * K + g["tid"], return_inverse=True, return_counts=True)
            U = int(uniq.shape[0])
            u_vid, u_tid = uniq // K, uniq % K
            u_lab = torch.zeros(U, dtype=torch.int64, device=dev).scatter_(0, inv, t["label"])   # (all members agree)
            by_tubelet = torch.sort(inv, stable=True).indices       # members by tubelet, then frame
            u_off = torch.zeros(U + 1, dtype=torch.int64, device=dev)
            u_off[1:] = torch.cumsum(u_len, 0)
            u_score = ops.tubelet_scores(t["score"][by_tubelet].contiguous(), u_off, tubelet_score == "max")
            # rank within (video, label): descending score, equal scores by ascending track id
            u_grp = u_vid * C + u_lab
            slots = flat.segment_order(u_score, u_grp)
            slot_of_u = torch.empty(U, dtype=torch.int64, device=dev)
            slot_of_u[slots] = torch.arange(U, device=dev)
            p_cnt = torch.bincount(u_grp, minlength=V * C)
            p_start = torch.cumsum(p_cnt, 0) - p_cnt
            u_rank = slot_of_u - p_start[u_grp]
            # the tasks: every (video, label) with a tubelet and a GT track, the most boxes first
            tk = v["tasks"].long()
            t_grp = vid_of_frame[tk[:, 1]] * C + tk[:, 0]
            keep = g["g_cnt"][t_grp] > 0
            tk, t_grp = tk[keep], t_grp[keep]
            T = int(tk.shape[0])
            match = torch.zeros((R, U), dtype=torch.uint8, device=dev)
            mgt = torch.full((R, U), -1, dtype=torch.int32, device=dev)
        if T:
            P, G = p_cnt[t_grp], g["g_cnt"][t_grp]
            PG = P * G
            pair_off = torch.cumsum(PG, 0) - PG
            big = PG > LDS_PAIRS
            wsz = torch.where(big, PG, torch.zeros_like(PG))
            ws_off = torch.where(big, torch.cumsum(wsz, 0) - wsz, torch.full_like(PG, -1))
            n_pairs, ws_pairs = (int(x) for x in torch.stack([PG.sum(), wsz.sum()]).tolist())
            tasks = torch.stack([tk[:, 0], tk[:, 1], tk[:, 2], p_start[t_grp], P, g["g_start"][t_grp], G,
                                 torch.zeros_like(P)], 1).to(torch.int32).contiguous()
            offs = torch.stack([pair_off, ws_off], 1).contiguous()
            res = ops.tubelet_match(t["box"][order].contiguous(), fid[order].to(torch.int32), u_rank[inv][order].to(torch.int32),
                                    v["seg_off"], g["ratio"], g["box"], g["track"], g["seg_off"], tasks, offs,
                                    slots.to(torch.int32), u_len.to(torch.int32), g["len"], thr, F, C, n_pairs, ws_pairs,
                                    want_pairs=True, return_workspace=return_workspace)
            match, mgt, hits, both = res[:4]
            out["ws_pairs"] = ws_pairs
            if return_workspace:
                out["workspace"] = tuple(a.cpu().numpy() for a in res[4])
        # AP: the detection AP's kernel over the tubelets, per label in descending score, equal scores by (video, id)
        if U:
            gorder = flat.segment_order(u_score, u_lab).to(torch.int32)
            lab_off = torch.zeros(C + 1, dtype=torch.int64, device=dev)
            lab_off[1:] = torch.cumsum(torch.bincount(u_lab, minlength=C), 0)
        else:
            gorder = torch.zeros(0, dtype=torch.int32, device=dev)
            lab_off = torch.zeros(C + 1, dtype=torch.int64, device=dev)
        ap = ops.vid_eval_ap(match, torch.zeros((R, U), dtype=torch.float64, device=dev), gorder, lab_off, n_pos)
        # the GT table: who took each GT track at the table's threshold, with the pair's hits and union
        taker = torch.full((J,), -1, dtype=torch.int64, device=dev)
        t_hits = torch.zeros(J, dtype=torch.int64, device=dev)
        t_union = torch.zeros(J, dtype=torch.int64, device=dev)
        if T:
            slot = mgt[table_threshold(thr)].long()
            w = torch.nonzero(slot >= 0).reshape(-1)
            grp_pair = torch.full((V * C,), -1, dtype=torch.int64, device=dev)
            grp_pair[t_grp] = pair_off
            sw, gw = slot[w], u_grp[w]
            idx = grp_pair[gw] + u_rank[w] * g["g_cnt"][gw] + (sw - g["g_start"][gw])
            taker[sw] = u_tid[w]
            t_hits[sw] = hits[idx].long()
            t_union[sw] = u_len[w] + g["len"][sw].long() - both[idx].long()
        host = {k: a.cpu().numpy() for k, a in (("vid", u_vid), ("tid", u_tid), ("lab", u_lab), ("len", u_len),
                                                 ("score", u_score), ("match", match), ("mgt", mgt), ("ap", ap),
                                                 ("taker", taker), ("hits", t_hits), ("union", t_union))}
        if T and pairs:
            host.update(tasks=tasks.cpu().numpy(), pair_off=pair_off.cpu().numpy(), slots=slots.cpu().numpy(),
                        all_hits=hits.cpu().numpy(), all_both=both.cpu().numpy())
    tub = np.zeros(U, TUBELET_DTYPE)
    for name, k in (("video", "vid"), ("id", "tid"), ("label", "lab"), ("count", "len"), ("score", "score")):
        tub[name] = host[k]
    out["tubelets"] = tub
    out["match"] = host["match"]
    slot_num = np.concatenate([gt["slot_num"], [-1]])            # (slot -1 -> number -1)
    out["matched_gt"] = slot_num[host["mgt"].astype(np.int64)]
    out["ap"] = host["ap"]
    table = np.zeros(J, GT_TABLE_DTYPE)
    table["video"], table["gt"], table["label"] = gt["slot_video"], gt["slot_num"], gt["slot_label"]
    table["count"], table["tubelet"], table["hits"], table["union"] = gt["len"], host["taker"], host["hits"], host["union"]
    out["gt_table"] = table
    if pairs:
        out["pairs"] = {}
        if T:
            for (c, f0, L, p0, P, g0, G, _), po in zip(host["tasks"].tolist(), host["pair_off"].tolist()):
                video = int(gt["slot_video"][g0])
                out["pairs"][(video, c)] = {"tubelets": host["tid"][host["slots"][p0:p0 + P]].tolist(),
                                            "gt": gt["slot_num"][g0:g0 + G].tolist(),
                                            "hits": host["all_hits"][po:po + P * G].reshape(P, G).astype(np.int64),
                                            "both": host["all_both"][po:po + P * G].reshape(P, G).astype(np.int64)}
    return out


def summarize(ap):
    """ap [R, C] -> (map [R]: the nanmean over the foreground labels 1 .. C-1, mean: the mean of the maps)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # nanmean of an all-NaN row is NaN
        maps = np.asarray([np.nanmean(row[1:]) if len(row) > 1 else np.nan for row in np.asarray(ap, np.float64)])
        return maps, float(np.mean(maps))


def format_result(thresholds, ap, classes=None):
    """The text of result_tubelets.txt."""
    classes = vid_eval.CLASSES if classes is None else classes
    maps, mean = summarize(ap)
    s = ""
    for (n, d), m in zip(thresholds, maps):
        s += "tubelet AP | tIoU>={:.2f} = {:0.4f}\n".format(n / float(d), m)
    s += "tubelet AP | mean       = {:0.4f}\n".format(mean)
    s += "Category AP:\n"
    for i, a in enumerate(np.asarray(ap)[table_threshold(thresholds)]):
        if i == 0:  # skip background
            continue
        s += "{:<16}: {:.4f}\n".format(classes[i] if i < len(classes) else str(i), a)
    return s


def evaluate_tracks(predictions, groundtruth, videos, thresholds=THRESHOLDS, tubelet_score="mean", output_folder=None,
                    device="cuda", logger=None):
    """Tubelet AP of `predictions` (list[BoxList] with "scores", "labels", "track_ids") against `groundtruth` (a
    vid_eval.VIDTrackGroundTruth of the same frames) over `videos` ((start, length) pairs); see the module docstring.
    -> {"thresholds", "ap" [R, C], "map" [R], "mean", "gt_table", "tubelets", "text"}; the text goes to the log and to
    <output_folder>/result_tubelets.txt."""
    r = run(predictions, groundtruth, videos, thresholds, tubelet_score, device, pairs=False)
    maps, mean = summarize(r["ap"])
    text = format_result(r["thresholds"], r["ap"])
    vid_eval.write_result(text, logger, "track_eval", output_folder, "result_tubelets.txt")
    return {"thresholds": r["thresholds"], "ap": r["ap"], "map": maps, "mean": mean, "gt_table": r["gt_table"],
            "tubelets": r["tubelets"], "text": text}
