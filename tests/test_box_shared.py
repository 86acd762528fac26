"""CPU: what the box kernels share -- the workspace byte counts of every entry point whose layout is carved by
csrc/workspace.h (pinned to the values of the hand-written formulas they replace), the -ffp-contract=off flag of every
translation unit that sees csrc/box_math.h, and flat.py's video-task layer on CPU tensors against hand-written values."""
import os
import re

import pytest
import torch

from mega.pytorch_amd import _lib, build, flat
from mega.pytorch_amd.structures import BoxList

CSRC = build.CSRC
AUG = [(1, 1, 1, 2), (2, 3, 100, 31), (1, 16, 512, 2), (3, 2, 77, 5)]        # (F, K, R, NC); the first: m = P = 1
# name -> [(arguments, bytes)]: recorded from the library before the layouts moved onto the carver.  Sizes that are no
# multiple of 256, the arguments that give 0, and for tracks max_open at the LDS table's 1024 entries and one beyond.
WORKSPACE_BYTES = {
    "mega_nms_workspace_bytes": [((1, 1), 512), ((1, 64), 768), ((1, 65), 1536), ((3, 100), 5120), ((2, 6000), 9024256),
                                 ((30, 1024), 3932416)],
    "mega_nms_full_workspace_bytes": [((1,), 1792), ((63,), 2816), ((64,), 2816), ((1000,), 153856), ((8192,), 8593920)],
    "mega_rpn_select_workspace_bytes": [((1, 1), 2048), ((3, 999), 471552), ((1, 6000), 4686848), ((2, 8192), 17252864)],
    "mega_postprocess_batched_workspace_bytes": [((1, 1, 2), 2816), ((3, 77, 5), 61696), ((1, 300, 31), 802816),
                                                 ((2, 1024, 31), 10875648)],
    "mega_postprocess_workspace_bytes": [((1, 2), 2816), ((77, 5), 21760), ((300, 31), 802816)],
    "mega_bbox_aug_merge_workspace_bytes": list(zip(AUG, (2304, 883456, 401920, 91648))),
    "mega_soft_merge_workspace_bytes": list(zip(AUG, (2816, 1243648, 565760, 128768))),
    "mega_vid_eval_workspace_bytes": [((0, 1, 1), 512), ((1, 1, 1), 512), ((1023, 3, 1), 512), ((1024, 3, 1), 512),
                                      ((5000, 31, 1), 768), ((1000, 31, 4), 1536), ((-1, 31, 4), 0), ((10, 0, 4), 0),
                                      ((10, 31, 0), 0)],
    "mega_seq_nms_workspace_bytes": [((1000, 60), 13568), ((1, 1), 1536), ((33, 7), 1792), ((1000, 1550), 37888),
                                     ((0, 10), 0), ((10, 0), 0), ((-5, 3), 0)],
    "mega_link_tracks_workspace_bytes": [((5, 1), 256), ((5, 1024), 256), ((5, 1025), 2048), ((1, 1025), 2048),
                                         ((7, 1500), 148480), ((5, 2024), 221696), ((0, 10), 0), ((10, 0), 0),
                                         ((-1, 5), 0)],
}


@pytest.mark.parametrize("name", sorted(WORKSPACE_BYTES))
def test_workspace_byte_counts_are_pinned(name):
    fn = getattr(_lib.load(), name)
    assert [(args, int(fn(*args))) for args, _ in WORKSPACE_BYTES[name]] == WORKSPACE_BYTES[name]


def test_workspace_byte_counts_by_hand():
    """Two of the pinned values derived from the layouts: every array rounded up to 256 bytes."""
    # Seq-NMS, N = 1000 boxes, 60 segments: S f64 [N] | P i32 [N] | fbS f64 [segs] | fbP, path_pos i32 [segs] | status
    assert dict(WORKSPACE_BYTES["mega_seq_nms_workspace_bytes"])[(1000, 60)] == 8192 + 4096 + 512 + 2 * 256 + 256 == 13568
    # tracks, 5 tasks, one open track beyond the LDS table each: seven arrays of 5 entries, then the status word
    assert dict(WORKSPACE_BYTES["mega_link_tracks_workspace_bytes"])[(5, 1025)] == 7 * 256 + 256


def _includes(path, seen):
    """The csrc headers a file includes with quotes, transitively."""
    for h in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
        if h not in seen and os.path.exists(os.path.join(CSRC, h)):
            seen.add(h)
            _includes(os.path.join(CSRC, h), seen)
    return seen


def _box_math_users():
    users = [src for src in build.SOURCES if "box_math.h" in _includes(os.path.join(CSRC, src), set())]
    assert set(users) >= {"boxes.hip", "bbox_aug.hip", "soft_nms.hip", "seq_nms.hip", "tracks.hip", "vid_eval.hip",
                          "proposal_recall.hip"}
    return users


def test_every_unit_that_sees_box_math_is_built_without_fma_contraction():
    for src in _box_math_users():
        assert "-ffp-contract=off" in build.SOURCES[src], src


def test_every_unit_that_sees_box_math_keeps_the_correctly_rounded_division():
    """box_iou1's quotient, and the one dev_suppresses_areas falls back to inside its 1e-5 band, must round like the host's
    (tests/test_box_boundary_gpu.py runs pairs whose decision hangs on that last bit).  hipcc's default is the correctly
    rounded expansion (-fhip-fp32-correctly-rounded-divide-sqrt); these flags trade it, or the signed zeros and separate
    roundings the kernels rely on, for speed -- none may reach such a unit, neither per file nor through BASE_FLAGS."""
    loose = {"-fno-hip-fp32-correctly-rounded-divide-sqrt", "-ffast-math", "-Ofast", "-funsafe-math-optimizations",
             "-freciprocal-math", "-fno-signed-zeros", "-fapprox-func", "-ffp-model=fast", "-ffp-model=aggressive",
             "-fgpu-approx-transcendentals"}
    for src in _box_math_users():
        flags = build.BASE_FLAGS + build.SOURCES[src]
        assert not loose & set(flags), (src, sorted(loose & set(flags)))


def _boxlist(rows):
    b = BoxList(torch.tensor([r[0] for r in rows], dtype=torch.float32).reshape(-1, 4), (640, 480))
    b.add_field("scores", torch.tensor([r[1] for r in rows], dtype=torch.float32))
    b.add_field("labels", torch.tensor([r[2] for r in rows], dtype=torch.int64))
    return b


def test_video_task_layer_on_cpu_tensors():
    """Three frames of 2, 0 and 3 boxes; videos of 1 and 2 frames; class 1 occurs only in the first video; boxes 2 and 4
    tie in score with box 3 between them.  Flat positions 0 .. 4 are the frame-by-frame concatenation."""
    box = [0, 0, 9, 9]
    preds = [_boxlist([(box, 0.5, 0), (box, 0.7, 1)]), _boxlist([]),
             _boxlist([(box, 0.3, 0), (box, 0.9, 0), (box, 0.3, 0)])]
    pk = flat.pack(preds, [(0, 1), {"start": 1, "seg_len": 2}], "seq_nms")
    assert (pk["F"], pk["N"], pk["C"]) == (3, 5, 2) and pk["counts"].tolist() == [2, 0, 3]
    cpu = torch.device("cpu")
    by_pos = flat.video_tasks(pk, cpu, by_score=False)
    by_score = flat.video_tasks(pk, cpu, by_score=True)
    for v in (by_pos, by_score):
        assert v["V"] == 2 and v["fid"].tolist() == [0, 0, 2, 2, 2]
        assert v["key"].tolist() == [0, 3, 2, 2, 2]                       # label * F + frame
        # segments (class 0: frames 0 1 2, class 1: frames 0 1 2) hold 1 0 3 | 1 0 0 boxes
        assert v["seg_off"].tolist() == [0, 1, 1, 4, 5, 5, 5] and v["seg_off"].dtype == torch.int64
        # (class, first frame, frames): class 0 in video 1 has 3 boxes; then the one-box tasks by class, then video;
        # class 1 has no box in video 1: no task
        assert v["tasks"].tolist() == [[0, 1, 2], [0, 0, 1], [1, 0, 1]] and v["tasks"].dtype == torch.int32
    assert by_pos["order"].tolist() == [0, 2, 3, 4, 1]                    # within a segment by position
    assert by_score["order"].tolist() == [0, 3, 2, 4, 1]                  # by descending score, the tie by position


def test_pack_error_texts_carry_the_callers_prefix():
    p = [_boxlist([([0, 0, 9, 9], 0.5, 0)])]
    with pytest.raises(ValueError, match=r"^tracks: the videos cover 2 frames, the predictions hold 1$"):
        flat.pack(p, [(0, 2)], "tracks")
    with pytest.raises(ValueError, match=r"^seq_nms: a prediction score is negative or NaN$"):
        flat.pack([_boxlist([([0, 0, 9, 9], -0.5, 0)])], [(0, 1)], "seq_nms")
