"""CPU: the demo's picture as tests/overlay_twin.py defines it (hand-computed pixel sets, the score text, the strict
threshold), the glyph atlas, tools/demo.py --dry-run, and VIDDemo's file handling with a stub detector and the twin in
place of the kernel."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import torch

import overlay_twin as tw
from mega.pytorch_amd import config, demo
from mega.pytorch_amd.structures import BoxList

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 12, 16
NAMES = ["bg", "a", "b"]
PAL = np.asarray([[0, 0, 0], [200, 30, 40], [10, 220, 90]], np.uint8)


class FlatAtlas(object):
    """every glyph one column wide, two rows high, coverage 0: a label is a solid 2-row bar, one pixel per character"""
    chars = demo.CHARSET
    cells = np.zeros((len(demo.CHARSET), 2, 1), np.uint8)
    advances = np.ones(len(demo.CHARSET), np.int32)


def _bg():
    return np.random.default_rng(0).integers(0, 256, (H, W, 3)).astype(np.uint8)


def _draw(rows, thickness=1, thr=0.5, bg=None, atlas=FlatAtlas):
    """rows: (box, score, class)"""
    bg = _bg() if bg is None else bg
    box = np.asarray([r[0] for r in rows], np.float32).reshape(-1, 4)
    score = np.asarray([r[1] for r in rows], np.float32)
    label = np.asarray([r[2] for r in rows], np.int64)
    return bg, tw.draw(bg, box, score, label, len(rows), (H, W), thr, thickness, PAL, atlas, NAMES)


def _expect(bg, picture):
    """'.' untouched, 'a' / 'b' the class colour of an outline, 'A' / 'B' a label pixel (coverage 0: the class colour)"""
    assert len(picture) == H and all(len(r) == W for r in picture)
    out = bg.copy()
    for y, row in enumerate(picture):
        for x, ch in enumerate(row):
            if ch != ".":
                out[y, x] = PAL[{"a": 1, "b": 2}[ch.lower()]]
    return out


def test_one_box_thickness_1():
    bg, got = _draw([((3, 4, 10, 9), 0.9, 1)])      # label "a: 0.90": 7 columns, rows 2-3, from column 3
    np.testing.assert_array_equal(got, _expect(bg, [
        "................",
        "................",
        "...AAAAAAA......",
        "...AAAAAAA......",
        "...aaaaaaaa.....",
        "...a......a.....",
        "...a......a.....",
        "...a......a.....",
        "...a......a.....",
        "...aaaaaaaa.....",
        "................",
        "................"]))
    black = np.zeros((H, W, 3), np.uint8)
    _, on_black = _draw([((3, 4, 10, 9), 0.9, 1)], bg=black)
    assert int((on_black != 0).any(2).sum()) == 14 + 8 + 8 + 4 + 4      # label, two rows of 8, two columns of 4 between


def test_one_box_thickness_3():
    bg, got = _draw([((3, 4, 10, 9), 0.9, 1)], thickness=3)
    np.testing.assert_array_equal(got, _expect(bg, [
        "................",
        "................",
        "...AAAAAAA......",
        "..aAAAAAAAaa....",
        "..aaaaaaaaaa....",
        "..aaaaaaaaaa....",
        "..aaa....aaa....",
        "..aaa....aaa....",
        "..aaaaaaaaaa....",
        "..aaaaaaaaaa....",
        "..aaaaaaaaaa....",
        "................"]))


def test_lower_score_wins_shared_pixels_and_labels_cover_outlines():
    # row 0 is the LOWER score: the order comes from the scores, not from the rows
    bg, got = _draw([((5, 6, 14, 11), 0.8, 2), ((1, 4, 8, 10), 0.9, 1)])
    np.testing.assert_array_equal(got, _expect(bg, [
        "................",
        "................",
        ".AAAAAAA........",
        ".AAAAAAA........",
        ".aaaaBBBBBBB....",
        ".a...BBBBBBB....",
        ".a...bbbbbbbbbb.",
        ".a...b..a.....b.",
        ".a...b..a.....b.",
        ".a...b..a.....b.",
        ".aaaabaaa.....b.",
        ".....bbbbbbbbbb."]))


def test_equal_scores_draw_in_row_order():
    _, got = _draw([((2, 5, 9, 9), 0.75, 1), ((2, 5, 9, 9), 0.75, 2)])
    assert (got[5, 2:10] == PAL[2]).all() and (got[3, 2:9] == PAL[2]).all()      # the later row is drawn last
    _, got = _draw([((2, 5, 9, 9), 0.75, 2), ((2, 5, 9, 9), 0.75, 1)])
    assert (got[5, 2:10] == PAL[1]).all() and (got[3, 2:9] == PAL[1]).all()


def test_label_that_would_leave_the_top_moves_inside_the_box():
    bg, got = _draw([((2, 1, 9, 6), 0.9, 1)])
    np.testing.assert_array_equal(got, _expect(bg, [
        "................",
        "..AAAAAAAa......",
        "..AAAAAAAa......",
        "..a......a......",
        "..a......a......",
        "..a......a......",
        "..aaaaaaaa......",
        "................",
        "................",
        "................",
        "................",
        "................"]))


def test_box_partly_outside_and_label_clamped_horizontally():
    bg, got = _draw([((-3, 5, 4, 20), 0.9, 1)])
    np.testing.assert_array_equal(got, _expect(bg, [
        "................",
        "................",
        "................",
        "AAAAAAA.........",
        "AAAAAAA.........",
        "aaaaa...........",
        "....a...........",
        "....a...........",
        "....a...........",
        "....a...........",
        "....a...........",
        "....a..........."]))
    bg, got = _draw([((12, 4, 15, 7), 0.9, 2)])      # the 7-column label ends at the right edge
    np.testing.assert_array_equal(got, _expect(bg, [
        "................",
        "................",
        ".........BBBBBBB",
        ".........BBBBBBB",
        "............bbbb",
        "............b..b",
        "............b..b",
        "............bbbb",
        "................",
        "................",
        "................",
        "................"]))


def test_boxes_wholly_outside_degenerate_or_without_a_colour_draw_nothing():
    for box in ((20, 2, 30, 8), (-9, -9, -2, -1), (2, 14, 8, 30), (8, 3, 5, 9), (3, 9, 8, 4)):
        bg, got = _draw([(box, 0.9, 1)], thickness=3)
        np.testing.assert_array_equal(got, bg)
    for cls in (-1, 3):
        bg, got = _draw([((3, 4, 10, 9), 0.9, cls)])
        np.testing.assert_array_equal(got, bg)


def test_zero_kept_detections_and_strict_threshold():
    bg, got = _draw([((3, 4, 10, 9), 0.3, 1), ((1, 1, 5, 5), 0.5, 2)], thr=0.5)
    np.testing.assert_array_equal(got, bg)
    thr = np.float32(0.7)
    bg, got = _draw([((3, 4, 10, 9), thr, 1)], thr=0.7)                   # equal to the threshold: not drawn
    np.testing.assert_array_equal(got, bg)
    bg, got = _draw([((3, 4, 10, 9), np.nextafter(thr, np.float32(1)), 1)], thr=0.7)
    assert (got != bg).any()
    # rows at and beyond `count` are not read
    box = np.asarray([[3, 4, 10, 9]] * 2, np.float32)
    got = tw.draw(bg, box, np.asarray([0.9, 0.9], np.float32), np.asarray([1, 2]), 0, (H, W), 0.5, 1, PAL, FlatAtlas, NAMES)
    np.testing.assert_array_equal(got, bg)


def test_rescale_is_one_f32_multiply_then_truncation():
    hw, rhw = (720, 1280), (562, 1000)
    sx, sy = tw.ratios(hw, rhw)
    assert sx == np.float32(1.28) and sy == np.float32(720 / 562) and sx.dtype == np.float32
    box = np.asarray([[100.0, 561.99, 781.25, 10.5], [-0.5, -1.0, 999.99, 0.7808]], np.float32)
    want = [[int(np.float32(v) * r) for v, r in zip(b, (sx, sy, sx, sy))] for b in box]
    np.testing.assert_array_equal(tw.rescale(box, sx, sy), want)
    assert tw.rescale(box, sx, sy)[1, 0] == 0 and tw.rescale(box, sx, sy)[1, 1] == -1      # toward zero


def test_label_blend_and_glyph_cells():
    class A(object):
        chars = demo.CHARSET
        cells = np.zeros((len(demo.CHARSET), 2, 3), np.uint8)
        advances = np.full(len(demo.CHARSET), 2, np.int32)
    A.cells[A.chars.index("a")] = [[255, 128, 77], [0, 1, 77]]        # the third column lies beyond the advance: not shown
    A.cells[A.chars.index("9")] = [[64, 0, 0], [0, 200, 0]]
    bg, got = _draw([((1, 6, 5, 9), 0.9, 1)], atlas=A)                   # "a: 0.90", 14 columns from x = 1, rows 4-5
    c = PAL[1].astype(int)

    def blend(a):
        return (c * (255 - a) + 255 * a + 127) // 255
    np.testing.assert_array_equal(got[4, 1], [255, 255, 255])
    np.testing.assert_array_equal(got[4, 2], blend(128))
    np.testing.assert_array_equal(got[5, 1], c)
    np.testing.assert_array_equal(got[5, 2], blend(1))
    np.testing.assert_array_equal(got[4, 3], c)                           # ':' is empty; the 77 column never shows
    x9 = 1 + 2 * "a: 0.90".index("9")
    np.testing.assert_array_equal(got[4, x9], blend(64))
    np.testing.assert_array_equal(got[5, x9 + 1], blend(200))
    assert (got[4:6, 1:15] != bg[4:6, 1:15]).any(2).all() and (got[4:6, 15] == bg[4:6, 15]).all()


SCORE_CASES = [0.125, 0.375, 0.625, 0.875, np.float32(0.705), np.float32(0.995), 0.9999, 1.0,
               np.float32(0.715), np.float32(0.815)]      # the last two: an f32 product rounds to 71.5 / 81.5, then to 72 / 82


def test_score_text_equals_python_formatting():
    want = {0: "0.12", 1: "0.38"}
    rng = np.random.default_rng(7)
    cases = [np.float32(s) for s in SCORE_CASES] + list(rng.random(10000, dtype=np.float32))
    wrong_in_f32 = 0
    for i, s in enumerate(cases):
        py = "%.2f" % float(s)
        assert tw.label_text("dog", s) == "dog: " + py
        assert tw.kernel_digits(s) == py, (float(s), tw.kernel_digits(s), py)
        if i in want:
            assert py == want[i]
        f32 = int(np.rint(np.float32(s) * np.float32(100.0)))
        wrong_in_f32 += "%d.%02d" % (f32 // 100, f32 % 100) != py
    assert wrong_in_f32 > 0      # why the product is taken in f64
    assert tw.label_text("dog", np.float32(0.0)) == "dog: 0.00" and tw.kernel_digits(0.0) == "0.00"


def test_glyph_atlas_and_palette():
    cells, adv, chars = demo.glyph_atlas(16)
    assert cells.dtype == np.uint8 and cells.ndim == 3 and cells.shape[0] == len(chars) == len(adv)
    assert (adv > 0).all() and (adv <= cells.shape[2]).all()
    need = set("".join(demo.CATEGORIES)) | set("0123456789:. ")
    assert need <= set(chars)
    for ch in need - {" "}:
        assert cells[chars.index(ch)].max() > 0, ch
    assert cells[chars.index(" ")].max() == 0
    assert demo.CATEGORIES[9] == "dog" and len(demo.CATEGORIES) == 31
    from mega.pytorch_amd import vid_eval
    assert demo.CATEGORIES is vid_eval.CLASSES
    atlas = demo.LabelAtlas(cells, adv, chars)
    assert atlas.class_glyphs.shape[0] == 31 and atlas.class_glyphs.shape[1] <= demo.MAX_NAME
    row = atlas.class_glyphs[10]
    assert "".join(chars[g] for g in row if g >= 0) == "domestic_cat"
    assert "".join(chars[g] for g in atlas.fmt_glyphs) == "0123456789: ."
    pal = demo.class_palette(31)
    assert pal.shape == (31, 3) and pal.dtype == np.uint8
    assert len({tuple(p) for p in pal[1:]}) == 30
    d = np.abs(pal[1:, None].astype(int) - pal[None, 1:].astype(int)).sum(2) + np.eye(30, dtype=int) * 999
    assert d.min() >= 24      # visibly distinct
    np.testing.assert_array_equal(pal, demo.class_palette(31))


def test_demo_cli_dry_run_prints_one_json_line_without_device_code(tmp_path):
    code = ("import sys, runpy\n"
            "sys.argv = ['demo.py', 'fgfa', '--arch', 'R-50', '--image-folder', 'frames', '--output-folder', 'out', "
            "'--threshold', '0.5', '--thickness', '3', '--dry-run']\n"
            "try:\n    runpy.run_path(%r, run_name='__main__')\nexcept SystemExit as e:\n    assert not e.code, e.code\n"
            "assert 'torch' not in sys.modules and 'mega.pytorch_amd' not in sys.modules\n"
            % os.path.join(ROOT, "tools", "demo.py"))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["dry_run"] is True and d["method"] == "fgfa" and d["arch"] == "R-50" and d["threshold"] == 0.5
    assert d["thickness"] == 3 and d["image_folder"] == "frames" and d["output_folder"] == "out" and d["suffix"] == ".JPEG"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "demo.py"), "mega", "--thickness", "2", "--dry-run"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0      # even thickness


def test_viddemo_on_cpu_with_a_stub_detector_and_the_twin(tmp_path):
    from PIL import Image
    H0, W0, L = 48, 80, 5
    rng = np.random.default_rng(3)
    names = ["000010.JPEG", "000002.JPEG", "000007.JPEG", "000001.JPEG", "000100.JPEG"]
    folder = tmp_path / "frames"
    folder.mkdir()
    for n in names:
        Image.fromarray(rng.integers(0, 256, (H0, W0, 3)).astype(np.uint8)).save(str(folder / n), format="JPEG", quality=90)
    (folder / "notes.txt").write_text("not a frame")
    cfg = config.get_cfg("R-50", "base")
    cfg.MODEL.DEVICE = "cpu"
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 60, 100
    seen = {}

    def runner(src, v):
        assert v["seg_len"] == L and src.in_hw == (H0, W0) and src.out_hw == (60, 100)
        seen["out_hw"] = src.out_hw
        r = np.random.default_rng(4)
        dets = []
        for t in range(L):
            n = [3, 0, 1, 4, 2][t]
            xy = r.uniform(0, [60, 30], (n, 2))
            b = BoxList(torch.from_numpy(np.concatenate([xy, xy + r.uniform(5, 30, (n, 2))], 1).astype(np.float32)).reshape(-1, 4),
                        (100, 60))
            b.add_field("scores", torch.from_numpy(r.uniform(0.5, 1.0, n).astype(np.float32)))
            b.add_field("labels", torch.from_numpy(r.integers(1, 31, n)))
            dets.append(b)
        return dets
    out = tmp_path / "out"
    d = demo.VIDDemo(cfg, confidence_threshold=0.7, thickness=3, output_folder=str(out), render_chunk=2, runner=runner,
                     overlay=tw.as_op(demo.CATEGORIES), source_kwargs={"workers": 2})
    frames = d.run_on_image_folder(str(folder))
    assert len(frames) == L and len(d.predictions) == L and [len(p) for p in d.predictions] == [3, 0, 1, 4, 2]
    drawn = 0
    for t, name in enumerate(sorted(names)):
        orig = np.asarray(Image.open(str(folder / name)).convert("RGB"))
        p = d.predictions[t]
        want = tw.draw(orig, p.bbox.numpy(), p.get_field("scores").numpy(), p.get_field("labels").numpy(), len(p), (60, 100),
                       0.7, 3, d.palette, d.atlas, demo.CATEGORIES)
        assert frames[t].dtype == np.uint8 and frames[t].shape == (H0, W0, 3)
        np.testing.assert_array_equal(frames[t], want)
        drawn += int((want != orig).any())
        path = out / ("%06d.jpg" % t)
        assert path.exists()
        assert Image.open(str(path)).size == (W0, H0)
        buf = io.BytesIO()
        Image.fromarray(frames[t]).save(buf, format="JPEG", quality=demo.JPEG_QUALITY)
        assert path.read_bytes() == buf.getvalue()
    assert drawn >= 2 and sorted(os.listdir(str(out))) == ["%06d.jpg" % t for t in range(L)]
    # generate_images on its own writes the same files
    d.output_folder = str(tmp_path / "again")
    d.generate_images(frames)
    for t in range(L):
        assert (tmp_path / "again" / ("%06d.jpg" % t)).read_bytes() == (out / ("%06d.jpg" % t)).read_bytes()
