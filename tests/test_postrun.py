"""CPU: the chain after the detections (mega/pytorch_amd/postrun.py) -- that tools/eval_vid.py's flags and inference()'s
keywords describe the same Plan, which stages a Plan runs, in which order and on which list (the stages replaced by
recorders: no device), and that the options that need detections are refused for proposals in both vocabularies."""
import importlib.util
import logging
import os

import pytest

from mega.pytorch_amd import diagnose, inference, motion_iou, postrun, seq_nms, track_eval, tracks, vid_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--predictions", "p.pth", "--img-index", "i.txt", "--anno-path", "a"]
G, T = "gt:VIDGroundTruth", "gt:VIDTrackGroundTruth"
RAW = "eval:raw:result.txt"
LOG = logging.getLogger("test_postrun")

# name: (the tool's flags, inference()'s keywords (None: the tool alone can ask for it), box_only / limit / recall_table as
# cfg.MODEL.RPN_ONLY and the tool give them, the stages of a run with annotations)
CASES = {
    "nothing": ([], {}, {}, [G, RAW]),
    "seq_nms": (["--seq-nms", "--seq-nms-link-iou", "0.6", "--seq-nms-iou", "0.4", "--seq-nms-rescore", "max"],
                {"seq_nms": {"link_iou": 0.6, "nms_iou": 0.4, "rescore": "max"}}, {},
                [G, RAW, "seq_nms:raw", "save:seq:predictions_seq_nms.pth", "eval:seq:result_seq_nms.txt"]),
    "tracks": (["--tracks"], {"tracks": True}, {},
               [G, RAW, "link:raw", "save:linked:predictions_tracks.pth", "write:tracks.txt"]),
    "tracks_rescore": (["--tracks", "--tracks-rescore", "max"], {"tracks": {"rescore": "max"}}, {},
                       [G, RAW, "link:raw", "save:linked:predictions_tracks.pth", "write:tracks.txt",
                        "eval:linked:result_tracks.txt"]),
    "tracks_refine": (["--tracks", "--tracks-fill", "--tracks-smooth", "2", "--tracks-fill-scale", "0.5"],
                      {"tracks": {"fill": True, "smooth": 2, "fill_scale": 0.5}}, {},
                      [G, RAW, "link:raw", "refine:linked", "save:refined:predictions_tracks.pth", "write:tracks.txt",
                       "eval:refined:result_tracks.txt"]),
    "tracks_tubelets": (["--tracks", "--tubelet-ap", "--tubelet-score", "max"],
                        {"tracks": {"tubelet_ap": True, "tubelet_score": "max"}}, {},
                        [T, RAW, "link:raw", "save:linked:predictions_tracks.pth", "write:tracks.txt", "tubelets:linked:max"]),
    "diagnose": (["--diagnose", "--diagnose-score-thresh", "0.3", "--diagnose-bg-thresh", "0.2"],
                 {"diagnose": {"score_thresh": 0.3, "bg_thresh": 0.2}}, {}, [G, RAW, "diagnose:raw"]),
    "derive": (["--motion-iou", "derive", "--motion-window", "7"], {"motion_iou": {"derive": True, "window": 7}}, {},
               [T, "derive:7", RAW + ":derived"]),
    "mat": (["--motion-iou", "m.mat"], {"motion_iou": "m.mat"}, {}, [G, "load:m.mat", RAW + ":loaded"]),
    "box_only": (["--box-only", "--limit", "25", "--recall-table"], {}, {"box_only": True, "limit": 25, "recall_table": True},
                 [G, "proposals:raw:25:(10, 50, 100, 300)"]),
    # beyond the table of front-end pairs: the wiring between the stages
    "seq_nms_then_tracks": (["--seq-nms", "--tracks"], {"seq_nms": True, "tracks": True}, {},
                            [G, RAW, "seq_nms:raw", "save:seq:predictions_seq_nms.pth", "eval:seq:result_seq_nms.txt",
                             "link:seq", "save:linked:predictions_tracks.pth", "write:tracks.txt"]),
    "tubelets_of_given_ids": (["--tubelet-ap"], None, {"tubelet_score": "mean"}, [T, RAW, "tubelets:raw:mean"]),
    "everything": (["--seq-nms", "--tracks", "--tracks-rescore", "avg", "--tracks-smooth", "1", "--tubelet-ap", "--diagnose",
                    "--motion-iou", "derive", "--save-motion-iou", "out.mat", "--cache", "gt.npz"],
                   None, {"seq_nms": True, "tracks": {"rescore": "avg", "smooth": 1, "tubelet_ap": True}, "diagnose": True,
                          "motion_iou": "derive", "save_motion_iou": "out.mat", "cache": "gt.npz"},
                   [T + ":gt.npz", "derive:10", "save_mat:out.mat", RAW + ":derived", "diagnose:raw", "seq_nms:raw",
                    "save:seq:predictions_seq_nms.pth", "eval:seq:result_seq_nms.txt:derived", "link:seq", "refine:linked",
                    "save:refined:predictions_tracks.pth", "write:tracks.txt", "eval:refined:result_tracks.txt:derived",
                    "tubelets:refined:mean"]),
}
EVALUATIONS = ("gt:", "derive:", "save_mat:", "load:", "eval:", "diagnose:", "proposals:", "tubelets:")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("eval_vid_tool", os.path.join(ROOT, "tools", "eval_vid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _plan(name):
    _, keywords, extra, _ = CASES[name]
    return postrun.plan(anno_path="a", **dict(keywords or {}, **extra))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_flags_and_the_keywords_give_the_same_plan(tool, name):
    args, plan = tool.build_plan(BASE + CASES[name][0])
    assert plan == _plan(name)
    assert args.predictions == "p.pth" and args.device == "cuda:0"
    with pytest.raises(AttributeError):
        plan.box_only = True


def test_a_plan_holds_every_default():
    plan = postrun.plan(seq_nms=True, tracks={"smooth": 1}, diagnose=True, motion_iou="derive", anno_path="nowhere")
    assert dict(plan.seq_nms) == {"link_iou": 0.5, "nms_iou": 0.3, "rescore": "avg"}
    assert dict(plan.tracks) == {"score_thresh": 0.05, "link_iou": 0.5, "max_gap": 1, "min_len": 1, "rescore": None}
    assert dict(plan.refine) == {"fill": False, "smooth": 1, "fill_scale": 1.0}
    assert dict(plan.diagnose) == {"score_thresh": diagnose.SCORE_THRESH, "bg_thresh": diagnose.BG_THRESH}
    assert plan.window == motion_iou.WINDOW and plan.motion_iou is None and plan.tubelet_score is None
    off = postrun.plan(seq_nms=False, tracks={"fill": False, "smooth": 0, "fill_scale": 0.5}, diagnose=None)
    assert off.seq_nms is None and off.refine is None and off.diagnose is None and off.window is None
    assert off.tracks == postrun.plan(tracks=True).tracks
    lists = [[0.5]]
    assert postrun.plan(motion_iou=lists).motion_iou is lists


def test_plan_checks_every_stage():
    for kw, msg in (({"seq_nms": {"link_iou": 2.0}}, "^seq_nms: link_iou"), ({"tracks": {"max_gap": -1}}, "^tracks: max_gap"),
                    ({"tracks": {"fill": "yes"}}, "^tracks: fill"), ({"diagnose": {"bg_thresh": 0.6}}, "^diagnose: bg_thresh"),
                    ({"tracks": {"tubelet_ap": True, "tubelet_score": "median"}}, "^track_eval: tubelet_score"),
                    ({"tubelet_score": "median"}, "^track_eval: tubelet_score"),
                    ({"motion_iou": {"derive": True, "window": 99}, "anno_path": "a"}, "^motion_iou: window"),
                    ({"motion_iou": "derive"}, "^motion_iou: deriving the table needs anno_path")):
        with pytest.raises(ValueError, match=msg):
            postrun.plan(**kw)


@pytest.mark.parametrize("option,keywords,flags,says,flag", [
    ("seq_nms", {"seq_nms": True}, ["--seq-nms"], "Seq-NMS rescoring (seq_nms=...) needs detections",
     "--seq-nms / --motion-iou apply to detections"),
    ("tracks", {"tracks": {"tubelet_ap": True}}, ["--tracks", "--tubelet-ap"], "track linking (tracks=...) needs detections",
     "--tracks applies to detections"),
    ("tubelet_ap", {"tubelet_score": "mean"}, ["--tubelet-ap"], "the tubelet AP (tubelet_ap) needs detections",
     "--tubelet-ap applies to tracks"),
    ("diagnose", {"diagnose": {"bg_thresh": 0.9}}, ["--diagnose"], "the error diagnosis (diagnose=...) needs detections",
     "--diagnose applies to detections")])
def test_what_needs_detections_is_refused_for_proposals(tool, capsys, option, keywords, flags, says, flag):
    with pytest.raises(postrun.ProposalOnly) as e:
        postrun.plan(box_only=True, **keywords)
    assert e.value.option == option and isinstance(e.value, ValueError)
    assert str(e.value) == "MODEL.RPN_ONLY returns proposals: " + says
    with pytest.raises(SystemExit) as e:
        tool.build_plan(BASE + ["--box-only"] + flags)
    assert e.value.code == 2
    assert "--box-only evaluates proposals: " + flag in capsys.readouterr().err


class Recorder(object):
    """Every stage postrun.run calls, replaced: `events` gets "stage:input list:what else matters", a list is the tag of the
    stage that made it."""

    def __init__(self, monkeypatch, tmp_path):
        self.events, self.kwargs, ev = [], {}, self.event

        def ground_truth(name):
            def make(img_index, anno_path, cache=None):
                assert (img_index, anno_path) == (str(tmp_path / "index.txt"), "anno")
                ev("gt", name, *([cache] if cache else []))
                return type(name, (object,), {"off": "offsets"})()
            return make

        def detections(preds, gt, motion_iou=None, result_name="result.txt", **kw):
            ev("eval", preds[0], result_name, *([motion_iou] if motion_iou else []), kw=kw)
            return {"evaluated": preds[0]}

        def stage(name, result, extra=lambda a, kw: []):
            def call(preds, *a, **kw):
                ev(name, preds[0], *extra(a, kw), kw=kw)
                return result
            return call
        monkeypatch.setattr(vid_eval, "VIDGroundTruth", ground_truth("VIDGroundTruth"))
        monkeypatch.setattr(vid_eval, "VIDTrackGroundTruth", ground_truth("VIDTrackGroundTruth"))
        monkeypatch.setattr(vid_eval, "load_motion_iou", lambda path: ev("load", path) or "loaded")
        monkeypatch.setattr(motion_iou, "derive", lambda gt, videos, window, device: ev("derive", window) or "derived")
        monkeypatch.setattr(motion_iou, "save_mat", lambda path, table, off: ev("save_mat", path, kw={"off": off, "table": table}))
        monkeypatch.setattr(vid_eval, "evaluate_detections", detections)
        monkeypatch.setattr(vid_eval, "evaluate_proposals",
                            stage("proposals", {"recall": 1.0}, lambda a, kw: [kw["limit"], kw["limits"]]))
        monkeypatch.setattr(diagnose, "evaluate_errors", stage("diagnose", {"text": "diagnosis"}))
        monkeypatch.setattr(seq_nms, "seq_nms", stage("seq_nms", ["seq"]))
        monkeypatch.setattr(tracks, "link", stage("link", (["linked"], "table")))
        monkeypatch.setattr(tracks, "refine", stage("refine", (["refined"], {"tracks": 1, "filled": 2})))
        monkeypatch.setattr(tracks, "format_table", lambda table: ev("write", "tracks.txt") or "text of the %s\n" % table)
        monkeypatch.setattr(track_eval, "evaluate_tracks",
                            stage("tubelets", {"text": "tubelets"}, lambda a, kw: [kw["tubelet_score"]]))
        monkeypatch.setattr(inference, "save_predictions", lambda preds, path: ev("save", preds[0], os.path.basename(path)))

    def event(self, name, *what, kw=None):
        self.events.append(":".join([name] + [str(w) for w in what]))
        self.kwargs[self.events[-1]] = kw

    def run(self, plan, tmp_path, anno=True, out="out"):
        (tmp_path / "index.txt").write_text("v 1 0 2\nv 2 1 2\nw 3 0 1\n")
        titles = []
        got = postrun.run(plan, ["raw"], str(tmp_path / "index.txt"), "anno" if anno else None, out and str(tmp_path / out), "dev",
                          logger=LOG, report=lambda title, result: titles.append(title))
        if "write:tracks.txt" in self.events:
            assert (tmp_path / out / "tracks.txt").read_text() == "text of the table\n"
        return got, titles


@pytest.mark.parametrize("anno", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_stages_and_their_order(monkeypatch, tmp_path, name, anno):
    """With annotations: the stages CASES lists, each on the list it names.  Without: the same run less every evaluation
    -- the lists are still made and written."""
    rec = Recorder(monkeypatch, tmp_path)
    plan = _plan(name)
    got, titles = rec.run(plan, tmp_path, anno)
    want = [e for e in CASES[name][3] if anno or not e.startswith(EVALUATIONS)]
    assert rec.events == want
    assert got["rescored"] == (["seq"] if plan.seq_nms else None)
    assert got["tracked"] == ((["refined"] if plan.refine else ["linked"]) if plan.tracks else None)
    assert got["table"] == ("table" if plan.tracks else None)
    assert got["refine_info"] == ({"tracks": 1, "filled": 2} if plan.refine else None)
    assert sum(e.startswith("gt:") for e in rec.events) == int(anno)               # parsed once, or never
    assert ("refine:linked" in rec.events) == (plan.refine is not None) == (name in ("tracks_refine", "everything"))
    for e, kw in rec.kwargs.items():
        if e.startswith(("eval:", "diagnose:", "proposals:", "tubelets:")):          # where the evaluations write and log
            assert (kw["output_folder"], kw["device"], kw["logger"]) == (str(tmp_path / "out"), "dev", LOG)
        elif e.startswith(("seq_nms:", "link:", "refine:")):
            assert kw["device"] == "dev"


def test_what_the_stages_are_given_and_what_is_reported(monkeypatch, tmp_path):
    rec = Recorder(monkeypatch, tmp_path)
    plan = postrun.plan(anno_path="anno", **CASES["everything"][2])
    _, titles = rec.run(plan, tmp_path)
    assert titles == ["", "Diagnosis", "Seq-NMS", "Tracks", "Tracks, rescored and refined", "Tubelets"]
    assert rec.kwargs["seq_nms:raw"] == {"device": "dev", "link_iou": 0.5, "nms_iou": 0.3, "rescore": "avg"}
    assert rec.kwargs["link:seq"] == {"device": "dev", "score_thresh": 0.05, "link_iou": 0.5, "max_gap": 1, "min_len": 1,
                                      "rescore": "avg"}
    assert rec.kwargs["refine:linked"] == {"device": "dev", "fill": False, "smooth": 1, "fill_scale": 1.0}
    assert rec.kwargs["diagnose:raw"]["motion_iou"] == "derived"
    assert {k: rec.kwargs["diagnose:raw"][k] for k in ("score_thresh", "bg_thresh")} == dict(plan.diagnose)
    assert rec.kwargs["save_mat:out.mat"] == {"off": "offsets", "table": "derived"}
    for name, want in (("tracks_rescore", ["", "Tracks", "Tracks, rescored"]), ("tracks_refine", ["", "Tracks", "Tracks, refined"]),
                       ("tracks", ["", "Tracks"]), ("box_only", ["Recall"])):
        assert Recorder(monkeypatch, tmp_path).run(_plan(name), tmp_path)[1] == want


def test_without_an_output_folder_nothing_is_written(monkeypatch, tmp_path):
    rec = Recorder(monkeypatch, tmp_path)
    rec.run(postrun.plan(anno_path="anno", **CASES["everything"][2]), tmp_path, out=None)
    assert rec.events == [e for e in CASES["everything"][3] if not e.startswith(("save:", "write:"))]
    assert all(kw["output_folder"] is None for e, kw in rec.kwargs.items() if e.startswith(("eval:", "tubelets:")))
    assert sorted(os.listdir(str(tmp_path))) == ["index.txt"]


def test_inference_plans_before_it_opens_anything():
    """The checks of inference() that are the chain's come from plan(), before the index file is opened or the model is
    looked at."""
    from mega.pytorch_amd import config
    cfg = config.get_cfg("R-50")
    with pytest.raises(ValueError, match="^seq_nms: rescore"):
        inference.inference(cfg, None, "nowhere", "nothing.txt", seq_nms={"rescore": "median"})
    cfg.MODEL.RPN_ONLY = True
    with pytest.raises(postrun.ProposalOnly, match="track linking"):
        inference.inference(cfg, None, "nowhere", "nothing.txt", tracks={"tubelet_ap": True})
