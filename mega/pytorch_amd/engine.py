"""Clip-level inference engine: the MI355X-first way to drive GeneralizedRCNNMEGA.

The reference's loop (mega_core/engine/inference.py:17-47) feeds one key frame per call and the model
runs 2-3 single-frame backbone passes per call.  Here the frame-independent stage (backbone -> RPN ->
res5 -> ROIAlign -> fc0; ~90 % of the FLOPs) of many upcoming frames is run as ONE batch
(large GEMM M, full chip), optionally sharded over the GPUs of a node (each rank computes a slice of the
batch, one RCCL all-gather of the fixed-size frame records over xGMI), and only then the inherently
sequential per-key-frame aggregation (global/local/memory relation attention, predictor, NMS) is stepped.
Results are identical to calling ``model(images)`` frame by frame: every kernel is batch-invariant.

Frame schedule = the reference's test-time feed (mega_core/data/datasets/vid_mega.py:95-142):
key frame 0 consumes local frames 0..12 and GLOBAL.SIZE shuffled global frames, key frame t > 0 consumes
local frame min(T-1, t+12) and one more global frame.

Pipeline (run()): two HIP streams.  The frame stage of batch b+1 (big MFMA kernels, enqueued with NO host
sync) runs concurrently with the aggregation steps of batch b (many small kernels that fill the CUs the
frame-stage tails leave idle).  The host only ever waits for work that was enqueued a full batch earlier
(proposal counts of batch b, detection counts of batch b-1).
"""
import os
from collections import deque

import numpy as np
import torch

from . import ops


def global_schedule(seg_len, global_size, seed=0, shuffle=True):
    """Frame order of a video for the global pool and the per-key-frame global frame ids (vid_mega.py:21-24,:112-120).
    shuffle = cfg.MODEL.VID.MEGA.GLOBAL.SHUFFLE (False: the reference's plain arange order)."""
    rng = np.random.RandomState(seed)
    shuffled = np.arange(seg_len)
    if shuffle:
        rng.shuffle(shuffled)

    def for_frame(idx):
        size = global_size if idx == 0 else 1
        return [int(shuffled[(idx + global_size - i - 1) % seg_len]) for i in range(size)]
    return for_frame


class _On(object):
    """`with _On(stream)`: run the block on that HIP stream; `_On(None)` is a no-op (CPU / single-stream mode)."""

    def __init__(self, s):
        self.s = s
        self.c = None

    def __enter__(self):
        if self.s is not None:
            self.c = torch.cuda.stream(self.s)
            self.c.__enter__()

    def __exit__(self, *a):
        if self.c is not None:
            self.c.__exit__(*a)


class KeyFrameShard(object):
    """Multi-GPU form of the batched aggregation (MEGAFeatureExtractor.aggregate_batch): key frame i of the video belongs
    to rank i mod world -- the rank that also ran the frame stage of FRAME i (ClipEngine.shard_plan), so the 225 proposal
    rows only the key frame's own aggregation reads (rows 75-299 of its record, generalized_rcnn_mega.py:154-158,:213-216)
    never leave the GPU that produced them.  `base` = the video index of the batch's first key frame: position t of the
    batch is key frame base + t.  What crosses ranks: per stage, the memory entries (75 / 15 / 15 feature rows) of every key
    frame of the batch -- one all-gather each -- and at the end the padded detections.  Nothing of the per-key-frame step is
    replicated.  `wire` (optional dict) accumulates the bytes this rank contributes to each collective."""

    def __init__(self, dist, group, rank, world, base=0, wire=None, order=None):
        self.dist, self.group, self.rank, self.world, self.base, self.wire = dist, group, rank, world, base, wire
        self.order = order                # optional list: the kinds of collectives in the order they were issued (tests)

    def owner(self, t):
        return (self.base + t) % self.world

    def _count(self, key, t):
        if self.wire is not None:
            self.wire[key] = self.wire.get(key, 0) + t.numel() * t.element_size()
        if self.order is not None:
            self.order.append(key)

    def gather_rows(self, own, nrows, like):
        """own {t: [n_t, D] rows of my key frames}, nrows[t] for ALL key frames -> list of [n_t, D] for all of them.
        (Packed by ONE block-copy launch: a slice assignment per key frame was 20 tiny launches per stage.)"""
        S, W = len(nrows), self.world
        per, R, D = (S + W - 1) // W, max(max(nrows), 1), like.shape[1]
        buf = like.new_zeros((per, R, D))
        ops.copy_blocks([(buf[t // W, :x.shape[0]], x) for t, x in own.items() if x.shape[0] > 0])
        out = torch.empty((W * per, R, D), dtype=like.dtype, device=like.device)
        self._count("memory_rows", buf)
        self.dist.all_gather_into_tensor(out, buf, group=self.group)
        return [out[self.owner(t) * per + t // W, :nrows[t]] for t in range(S)]

    def gather_detections(self, outs, S, max_det, device):
        """outs[t] = PostProcessor.run output of my key frames (None elsewhere) -> the same for all S key frames.
        A frame travels as cap2 = 2 * DETECTIONS_PER_IMG rows of (box [4] f32, score f32, label i64) + its count (the
        reference's cut keeps at most DETECTIONS_PER_IMG plus score ties, box_head/inference.py:139-148), packed into one
        byte buffer by ONE block-copy launch (round 3: four slice assignments per key frame).  A frame with more than cap2
        detections (> DETECTIONS_PER_IMG exact score ties at the cut) cannot travel whole: its true count is sent, and
        ClipEngine.run raises when it reads a count larger than the rows it holds -- never a silent truncation.  Note the
        padded shape differs from the single-GPU path's [(NC-1) * R] rows; only [:count] is used."""
        W = self.world
        per, cap2 = (S + W - 1) // W, 2 * max_det
        nb_box, nb_sc, nb_lab = cap2 * 16, cap2 * 4, cap2 * 8
        rec = nb_box + nb_sc + nb_lab + 16
        buf = torch.zeros((per, rec), dtype=torch.uint8, device=device)
        pairs = []
        for t, o in enumerate(outs):
            if o is None:
                continue
            ob, os_, ol, oc = o[:4]
            n = min(cap2, ob.shape[0])
            row = buf[t // W:t // W + 1]
            pairs.append((row[:, :n * 16], ob[:n].reshape(1, -1).view(torch.uint8)))
            pairs.append((row[:, nb_box:nb_box + n * 4], os_[:n].reshape(1, -1).view(torch.uint8)))
            pairs.append((row[:, nb_box + nb_sc:nb_box + nb_sc + n * 8], ol[:n].reshape(1, -1).view(torch.uint8)))
            pairs.append((row[:, nb_box + nb_sc + nb_lab:nb_box + nb_sc + nb_lab + 4], oc.reshape(1, -1).view(torch.uint8)))
        ops.copy_blocks(pairs)      # (the TRUE count travels: finish() raises if it exceeds the rows sent)
        out = torch.empty((W * per, rec), dtype=torch.uint8, device=device)
        self._count("detections", buf)
        self.dist.all_gather_into_tensor(out, buf, group=self.group)
        # four typed tensors (one bulk copy each): detections handed to the caller must own plainly-typed storage
        n_all = W * per
        ab = out[:, :nb_box].contiguous().view(torch.float32).view(n_all, cap2, 4)
        asc = out[:, nb_box:nb_box + nb_sc].contiguous().view(torch.float32).view(n_all, cap2)
        al = out[:, nb_box + nb_sc:nb_box + nb_sc + nb_lab].contiguous().view(torch.int64).view(n_all, cap2)
        ac = out[:, nb_box + nb_sc + nb_lab:nb_box + nb_sc + nb_lab + 4].contiguous().view(torch.int32).view(n_all, 1)
        res = []
        for t in range(S):
            g = self.owner(t) * per + t // W
            res.append((ab[g], asc[g], al[g], ac[g]))
        return res


class ClipEngine(object):
    def __init__(self, model, steps_per_batch=8, dist_group=None, overlap=True, graphs=True, reuse_records=False,
                 static_aggregation=False, keep_logits=False, batch_aggregation=True, ramp=False, frame_model=None,
                 graph_aggregation=True):
        """steps_per_batch: key-frame steps whose frame jobs are computed in one frame-stage batch
        (steady state: 2 frames per step).  dist_group: torch.distributed group to shard the frame stage over
        (None = single process).  overlap: use the two-stream pipeline (see module docstring).
        graphs: replay the frame stage from a hipGraph once a batch shape repeats.
        reuse_records: keep every frame's record (0.6 MB) for the rest of the video.  A frame is consumed twice --
        once entering the local window, once entering the global pool (vid_mega.py:104-120) -- and the reference
        runs backbone + RPN + res5 + fc0 both times; the record is a pure function of the frame, so the second
        use can take the stored one (first 75 rows for the global role).  Identical detections, ~half the frame-stage
        work over a whole video.  Off by default: the benchmark's headline keeps the reference's two passes."""
        self.model = model
        # frame_model: a second detector with the same weights in another compute dtype that runs the frame stage
        # (backbone .. fc0); `model` then only aggregates, on records cast to its dtype.  Mixed-precision runs: which
        # half of the path a bf16 deviation comes from (tests/test_e2e_gpu.py::test_r101_bf16_attribution).
        self.frame_model = model if frame_model is None else frame_model
        self.steps_per_batch = steps_per_batch
        self.group = dist_group
        if dist_group is not None:
            import torch.distributed as dist
            self.dist = dist
            self.rank, self.world = dist.get_rank(dist_group), dist.get_world_size(dist_group)
        else:
            self.dist, self.rank, self.world = None, 0, 1
        import os as _os      # diagnostics: take the sharded (all-gather) branch even with one rank
        self.force_sharded = dist_group is not None and _os.environ.get("MEGA_FORCE_SHARDED") == "1"
        self.mean = tuple(model.cfg.INPUT.PIXEL_MEAN)
        self.to_bgr = bool(model.cfg.INPUT.TO_BGR255)
        self.overlap = overlap
        self.use_graphs = graphs
        self._fgraphs = {}
        self._graph_pool = None
        self._graph_pool_r = None          # res5 graphs (replayed beside the RPN branch): their own pool and stream
        self._res5_stream = None
        self.reuse_records = reuse_records
        self.frames_per_launch = steps_per_batch + 2      # reuse_records: fixed frame-stage launch size
        fe = getattr(getattr(getattr(model, "roi_heads", None), "box", None), "feature_extractor", None)
        # static_aggregation (opt-in, diagnostic): every key frame after the cold start is its own aggregation batch of ONE
        # step, in steady state on fixed-address state and replayed from one hipGraph per key frame (RDN has no batched
        # path: per-frame steps)
        self._static = None
        if static_aggregation and hasattr(fe, "aggregate_batch"):
            self._static = StaticBatchAggregation(model, 1, use_graph=graphs, keep_keys=keep_logits)
        self.use_static = True            # False: aggregate eagerly on the model's deques (instrumented passes)
        # graph_aggregation (round 4, default with graphs + batched aggregation, single process): in steady state -- all
        # pools full, every frame with all its proposals -- the BATCHED aggregation of a step-batch (prepare_batch +
        # step_batch: ~100 launches, ~6 ms of Python) runs on fixed-address state and is replayed from one hipGraph.
        # Created at the first full step-batch, and only on an engine without _static (see run(): batched and use_static)
        self._sbatch = None
        self.graph_aggregation = bool(graph_aggregation and graphs)
        # batch_aggregation: the aggregation of all key frames of a step-batch runs stage by stage over the whole batch
        # (model.step_batch: projections / stage FCs as one GEMM each); off = one model.step() per key frame
        self.batch_aggregation = batch_aggregation and hasattr(fe, "aggregate_batch")      # (RDN: per-frame steps)
        # multi-GPU wire format: with the batched aggregation a key frame is aggregated by ONE rank, the one
        # that ran its frame stage, and only the base_num rows every window reads travel (shard_plan / records_async)
        self.owner_aligned = bool(self.batch_aggregation and static_aggregation is False and hasattr(model, "base_num")
                                  and getattr(fe, "cache_memory_kv", False))
        self.wire = {}                    # bytes this rank contributed to each kind of collective (tests, diagnostics)
        # and the kinds in issue order, with "aggregate" marking the start of a step-batch's aggregation (tests: a batch's
        # frame records are gathered before it is aggregated) -- a diagnostic: bounded, so that a long multi-GPU run does not
        # grow it without end
        self.wire_order = deque(maxlen=4096)
        self.group_agg = dist_group       # the aggregation's collectives run on another stream than the frame stage's:
        if dist_group is not None and self.world > 1:      # their own communicator
            # (the members are the ranks of dist_group itself -- a sub-group's global ranks are not 0 .. world-1 -- and
            #  new_group() is a collective over the DEFAULT group: every process must construct its engine)
            self.group_agg = self.dist.new_group(self.dist.get_process_group_ranks(dist_group))
        # ramp: every run() call is its own pipeline fill / drain (the first batch's frame stage and the last batch's
        # aggregation have nothing to overlap with).  With ramp=True a call's key frames are split into a SHORT first
        # and last batch (steps_per_batch // 4) around equal middle batches, so the un-overlapped head and tail shrink
        # (results are unchanged: every kernel is batch-invariant).  Each distinct batch size is its own hipGraph.
        self.ramp = ramp
        self.keep_logits = keep_logits    # tests: logits_log[i] = predictor class logits of the i-th key frame stepped
        self.logits_log = []
        self.key_boxes_log = []           # and the key frame's proposal boxes (rows of logits_log[i])
        self.key_index_log = []           # and their flat anchor indices (only with model.rpn.keep_index)
        self.static_steps = 0
        self._rec_cache = {}              # frame id -> record (reuse_records)
        self._rec_pending = set()         # frame ids whose record is being computed by an enqueued batch
        self.frames_computed = 0
        self.graph_stats = {"eager": 0, "captured": 0, "replayed": 0}
        self._streams = None
        # host-side seconds spent enqueuing / waiting, accumulated over run() calls (diagnostics for bench.py)
        self.host_times = {"frame_enqueue": 0.0, "aggregate_enqueue": 0.0, "frame_wait": 0.0, "finish_wait": 0.0, "steps": 0}

    # ------------------------------------------------------------------ state report (bench.py, tests)
    def static_replays(self):
        return 0 if self._static is None else self._static.replays

    def steady_state(self):
        """{"pools_full", "graphs_warm", "steady"}: pools_full = the local window, the global pool and the memory
        deques of every stage hold their maximum number of entries (SURVEY.md 8d steady state); graphs_warm = the
        steady frame-stage batch shape (and the aggregation step, with static aggregation) has been captured and
        replayed at least once, i.e. no eager batch / capture is still ahead."""
        m = self.model
        fe = m.roi_heads.box.feature_extractor
        if self._static is not None and self._static.active:
            full = True                   # StaticBatchAggregation.ready() only admits full pools
        else:
            full = hasattr(m, "records") and len(m.records) == m.all_frame_interval
            if full and getattr(m, "global_enable", False):
                full = len(fe.global_queue_list[0]["feats"]) == fe.global_size
            if full and getattr(m, "memory_enable", False):
                full = all(len(q["rois"]) == fe.all_frame_interval for q in fe.mem_queue_list)
        warm = True
        if self.use_graphs:
            warm = self.graph_stats["replayed"] >= 1
            if self._static is not None and self.use_static:
                warm = warm and self._static.replays >= 1
            if self._sbatch is not None and self._sbatch.active:
                warm = warm and self._sbatch.replays >= 1
        return {"pools_full": bool(full), "graphs_warm": bool(warm), "steady": bool(full and warm)}

    # ------------------------------------------------------------------ schedule
    def batch_sizes(self, n):
        """Key frames per batch for a run() call of n (non-cold-start) key frames."""
        spb = self.steps_per_batch
        if n <= 0:
            return []
        if not self.ramp or n <= spb:
            return [spb] * (n // spb) + ([n % spb] if n % spb else [])
        r = max(1, spb // 4)
        tail = r if n - r > r else 0
        mid = n - r - tail
        k = -(-mid // spb)
        sizes = [r] + [mid // k + (1 if i < mid % k else 0) for i in range(k)] + ([tail] if tail else [])
        return [x for x in sizes if x > 0]

    def jobs_for_step(self, idx, T, gfor):
        """[(frame_id, want, role)] consumed by key frame idx, in consumption order."""
        m = self.model
        if idx == 0:
            loc = [0]
            end = 0
            for _ in range(m.all_frame_interval - m.key_frame_location - 1):
                end = min(end + 1, T - 1)
                loc.append(end)
        else:
            loc = [min(T - 1, idx + m.all_frame_interval - m.key_frame_location - 1)]
        jobs = [(f, m.key_num, "l") for f in loc]
        if m.global_enable:
            jobs += [(f, m.base_num, "g") for f in gfor(idx)]
        return jobs

    # ------------------------------------------------------------------ frame stage (optionally sharded)
    class _RawFrames(object):
        """uint8 frames [n,H,W,3] whose preprocessing is still to run: the frame stage's graph path lets the
        preprocess kernel write straight into the graphs' static input (no 288 MB staging copy per 40-frame batch)."""

        def __init__(self, u8, mean, to_bgr):
            self.u8, self.mean, self.to_bgr = u8, mean, to_bgr
            n, h, w, _ = u8.shape
            self.shape, self.dtype, self.is_cuda, self.device = (n, 3, h, w), torch.float32, u8.is_cuda, u8.device

        def materialize(self, out=None):
            return ops.preprocess_frames(self.u8, self.mean, self.to_bgr, out=out)

    def _frames(self, clip, ids):
        """clip: uint8 [T,H,W,3] (device) -> preprocessed f32 [n,3,H,W] (as _RawFrames: preprocessing deferred to the
        frame stage); or already-preprocessed f32 [T,3,H,W]; or a feed.FrameSource (decodes on host threads, resizes
        on the device)."""
        if hasattr(clip, "fetch"):
            return self._RawFrames(clip.fetch(list(ids)).contiguous(), self.mean, self.to_bgr)
        if clip.is_cuda:   # pinned + non_blocking: the host must not wait for the work already queued on the stream
            idx = torch.tensor(ids, dtype=torch.int64).pin_memory().to(clip.device, non_blocking=True)
        else:
            idx = torch.as_tensor(ids)
        sel = clip.index_select(0, idx)
        if clip.dtype == torch.uint8:
            return self._RawFrames(sel.contiguous(), self.mean, self.to_bgr)
        return sel.contiguous()

    def _frame_stage(self, imgs, want, on_counts=None):
        """model.frame_stage_a + frame_stage_b, replayed from hipGraphs when this exact batch shape has been seen before.
        The frame stage is ~130 launches of static shape per batch: as graphs the host pays two replays (microseconds)
        instead of ~35 us of Python + ctypes per launch.  First occurrence of a shape runs eagerly (warm-up: packs
        weights, sets kernel attributes, fills the allocator), the second is captured.
        on_counts(cnt): called between the two halves with the device-side proposal counts (a fresh tensor): the caller
        starts their copy to the host there -- the counts are all the host needs to lay out the aggregation, and they
        exist 40 % of the stage before its features do."""
        m = self.frame_model
        raw = imgs if isinstance(imgs, self._RawFrames) else None
        # bf16 mode on the device: the stem reads the uint8 frames itself (preprocessing on its patch load: no f32 image
        # in HBM, no preprocess launch -- same bits); everything else gets the preprocessed f32 batch
        from .modeling import compute_dtype
        u8 = (raw is not None and raw.is_cuda and compute_dtype(m.cfg) in (torch.bfloat16, torch.float16)
              and getattr(m, "stem_reads_u8", False))
        norm = (raw.mean, raw.to_bgr) if u8 else None

        def stage_a(x):
            if u8:
                return m.frame_stage_a1(m.frame_stage_a0(x, norm), raw.shape[3], raw.shape[2])
            return m.frame_stage_a(x)
        if not (self.use_graphs and imgs.is_cuda):
            a = stage_a(raw.u8 if u8 else (raw.materialize() if raw is not None else imgs))
            if on_counts is not None:
                on_counts(a["cnt"])
            return m.frame_stage_b(a, want)
        # (u8 is part of the key: a uint8 clip on the fused-u8 stem path and a preprocessed f32 batch of the same size
        #  report the same shape and dtype but own different static inputs and graphs -- ADVICE r04)
        key = (tuple(imgs.shape), tuple(int(w) for w in want), imgs.dtype, bool(u8))
        ent = self._fgraphs.get(key)
        if ent is None:
            self._fgraphs[key] = {}
            self.graph_stats["eager"] += 1
            a = stage_a(raw.u8 if u8 else (raw.materialize() if raw is not None else imgs))
            if on_counts is not None:
                on_counts(a["cnt"])
            return m.frame_stage_b(a, want)
        if "graph" not in ent:
            ent["static_in"] = raw.u8.clone() if u8 else (raw.materialize() if raw is not None else imgs.clone())
            torch.cuda.current_stream().synchronize()
            if self._graph_pool is None:          # all frame-stage graphs replay one after the other on one stream:
                self._graph_pool = torch.cuda.graph_pool_handle()    # they can share one activation pool
            # thread-local capture mode: the RCCL watchdog thread of a multi-GPU run polls its events with
            # hipEventQuery, which the default (global) mode forbids on ANY thread while a capture is open
            # Four graphs: a0 backbone -> a1 RPN branch -> (counts) -> b2 ROIAlign + fc0 on this stream, b1 (res5, which
            # needs C4 only) on a side stream beside a1: the proposal selection at the end of a1 is one block per frame
            # (40 blocks on 256 CUs, ~0.4 ms per 40-frame batch) and disappears under res5's convolutions.  b1 runs
            # CONCURRENTLY with a1, so its temporaries live in a pool of their own (graphs sharing a pool must replay one
            # after the other); c4 and x5 are graph outputs kept alive here, never recycled.
            if self._graph_pool_r is None:
                self._graph_pool_r = torch.cuda.graph_pool_handle()
                self._res5_stream = torch.cuda.Stream(device=imgs.device)
            g0, g1, gr, gb = (torch.cuda.CUDAGraph() for _ in range(4))
            W, H = imgs.shape[3], imgs.shape[2]
            with torch.cuda.graph(g0, pool=self._graph_pool, capture_error_mode="thread_local"):
                ent["c4"] = m.frame_stage_a0(ent["static_in"], norm) if u8 else m.frame_stage_a0(ent["static_in"])
            with torch.cuda.graph(g1, pool=self._graph_pool, capture_error_mode="thread_local"):
                ent["a"] = m.frame_stage_a1(ent["c4"], W, H)
            with torch.cuda.graph(gr, pool=self._graph_pool_r, capture_error_mode="thread_local"):
                ent["x5"] = m.frame_stage_b1(ent["c4"])
            with torch.cuda.graph(gb, pool=self._graph_pool, capture_error_mode="thread_local"):
                ent["st"] = m.frame_stage_b2(ent["x5"], ent["a"], want)
            ent["graph_a0"], ent["graph_a1"], ent["graph_b1"], ent["graph"] = g0, g1, gr, gb
            ent["e0"], ent["e1"] = torch.cuda.Event(), torch.cuda.Event()
            self.graph_stats["captured"] += 1
        cur = torch.cuda.current_stream()
        if u8:
            ent["static_in"].copy_(raw.u8)              # 1.8 MB per frame (the f32 image was 7.2 MB)
        elif raw is not None:
            raw.materialize(out=ent["static_in"])       # (the capture batch: written twice, once)
        else:
            ent["static_in"].copy_(imgs)
        ent["graph_a0"].replay()
        ent["e0"].record(cur)
        side = self._res5_stream
        side.wait_event(ent["e0"])
        with torch.cuda.stream(side):
            ent["graph_b1"].replay()
            ent["e1"].record(side)
        ent["graph_a1"].replay()
        cnt = ent["a"]["cnt"].clone()
        if on_counts is not None:
            on_counts(cnt)
        cur.wait_event(ent["e1"])
        ent["graph"].replay()
        self.graph_stats["replayed"] += 1
        st = ent["st"]
        # the graph's outputs are overwritten by the next replay: hand out copies (6 MB per 16-frame batch)
        out = {"props": st["props"].clone(), "scores": st["scores"].clone(), "cnt": cnt,
               "feats": st["feats"].clone(), "want": st["want"]}
        if "index" in st:
            out["index"] = st["index"].clone()
        return out

    def shard_plan(self, jobs, rank=None, world=None):
        """How a frame-stage batch is dealt to the ranks.  -> (plan, mine).

        Owner-aligned form (the batched aggregation): local-window frame f goes to rank f mod world -- the
        rank that aggregates KEY FRAME f twelve steps later (KeyFrameShard.owner), so only the 75 rows every rank's window
        needs travel and rows 75-299 stay where they were computed; global-pool frames (75 rows) are dealt round-robin.
        Every rank runs ONE launch of nl local + ng global frames (short lists padded by repeating a job of that kind; a
        padded slot's record is never consumed).  plan = {"place": [(rank, slot in that rank's launch)] per job, "nl", "ng"},
        mine = positions (into jobs) this rank computes, in launch order (locals, then globals).
        Legacy form (per-frame aggregation: every rank steps every key frame and needs whole records): jobs grouped by row
        count, each group cut into contiguous slices; plan = [(want, positions, slice length, first slot)].
        The ONE definition of the dealing: records_async and the host-side prefetch both use it."""
        rank = self.rank if rank is None else rank
        world = self.world if world is None else world
        if not self.owner_aligned:
            groups = {}
            for pos, j in enumerate(jobs):
                groups.setdefault(int(j[1]), []).append(pos)
            plan, mine = [], []
            for want, poss in sorted(groups.items(), reverse=True):
                per = (len(poss) + world - 1) // world
                padded = poss + [poss[-1]] * (per * world - len(poss))
                plan.append((want, poss, per, len(mine)))
                mine += padded[rank * per:(rank + 1) * per]
            return plan, mine
        loc = [[] for _ in range(world)]
        glo = [[] for _ in range(world)]
        ng_seen = 0
        for pos, j in enumerate(jobs):
            if j[2] == "g":
                glo[ng_seen % world].append(pos)
                ng_seen += 1
            else:
                loc[int(j[0]) % world].append(pos)
        nl, ng = max(len(x) for x in loc), max(len(x) for x in glo)
        place = [None] * len(jobs)
        launches = []
        for r in range(world):
            for lst, n in ((loc[r], nl), (glo[r], ng)):
                if len(lst) < n:      # pad: a job of the same kind (its record lands in a slot nobody reads)
                    same = lst or next(x for x in (loc if lst is loc[r] else glo) if x)
                    lst = lst + [same[-1]] * (n - len(lst))
                launches.append(lst)
        for r in range(world):
            l, g = launches[2 * r], launches[2 * r + 1]
            for slot, pos in enumerate(loc[r]):
                place[pos] = (r, slot)
            for slot, pos in enumerate(glo[r]):
                place[pos] = (r, nl + slot)
        mine = launches[2 * rank] + launches[2 * rank + 1]
        return {"place": place, "nl": nl, "ng": ng}, mine

    @staticmethod
    def count_index(plan, njobs, nm):
        """Where job p's proposal count sits in the all-gathered count vector [world x nm] (nm = frames per rank and
        launch)."""
        if isinstance(plan, dict):
            return [r * nm + slot for r, slot in plan["place"]]
        idx = [0] * njobs
        for _, poss, per, first in plan:
            for slot, pos in enumerate(poss):
                idx[pos] = (slot // per) * nm + first + slot % per
        return idx

    def _count_wire(self, key, t):
        self.wire[key] = self.wire.get(key, 0) + t.numel() * t.element_size()
        self.wire_order.append(key)

    def records_async(self, clip, jobs, on_counts=None):
        """Enqueue the frame stage for jobs [(frame_id, want, role)]; no host sync.  -> handle for
        records_resolve().  on_counts: see _frame_stage; in the sharded path the ranks' counts are all-gathered between the
        two halves of the frame stage (one tiny collective) and handed to on_counts in job order."""
        if self.world == 1 and not self.force_sharded:
            return {"st": self._frame_stage(self._frames(clip, [j[0] for j in jobs]), [j[1] for j in jobs], on_counts)}
        plan, mine = self.shard_plan(jobs)
        mine_ids = [jobs[p][0] for p in mine]
        mine_want = [int(jobs[p][1]) for p in mine]
        early = None
        if on_counts is not None:
            def early(c):      # this rank's counts -> every rank, re-ordered to job order (index table cached per plan)
                nm = c.shape[0]
                sig = (tuple((int(j[0]) % self.world, int(j[1]), j[2]) for j in jobs), self.world, str(c.device))
                tab = getattr(self, "_cnt_index", None)
                if tab is None or tab[0] != sig:
                    tab = self._cnt_index = (sig, torch.tensor(self.count_index(plan, len(jobs), nm), dtype=torch.int64,
                                                               device=c.device))
                allc = torch.empty((self.world * nm,), dtype=c.dtype, device=c.device)
                self._count_wire("counts", c)
                self.dist.all_gather_into_tensor(allc, c.contiguous(), group=self.group)
                on_counts(allc.index_select(0, tab[1]))
        st = self._frame_stage(self._frames(clip, mine_ids), mine_want, early)
        dev, D, fdt = st["props"].device, st["feats"].shape[1], st["feats"].dtype
        esz = st["feats"].element_size()
        if isinstance(plan, dict):
            # ---- owner-aligned: every frame contributes ONE record of the rows every rank's window reads -- base_num (75)
            # boxes, scores and feature rows + its count -- whatever its role; the whole batch travels in ONE all-gather of
            # a packed byte buffer.  Packed by one block-copy launch (mega_copy_segments); the receivers' records are VIEWS
            # of the gathered buffer.  Rows base_num .. key_num - 1 of a local frame stay on this rank: only key frame f's
            # aggregation reads them, and this rank owns it.
            bn = self.model.base_num
            nb_box, nb_sc, nb_feat = bn * 16, (bn * 4 + 15) // 16 * 16, bn * D * esz
            rec_bytes = nb_box + nb_sc + nb_feat + 16
            nrec = plan["nl"] + plan["ng"]
            buf = torch.zeros((nrec, rec_bytes), dtype=torch.uint8, device=dev)
            pairs, row = [], 0
            for slot, w in enumerate(mine_want):
                pairs.append((buf[slot:slot + 1, :nb_box], st["props"][slot, :bn].reshape(1, -1).view(torch.uint8)))
                pairs.append((buf[slot:slot + 1, nb_box:nb_box + bn * 4], st["scores"][slot, :bn].reshape(1, -1).view(torch.uint8)))
                pairs.append((buf[slot:slot + 1, nb_box + nb_sc:nb_box + nb_sc + nb_feat],
                              st["feats"][row:row + bn].reshape(1, -1).view(torch.uint8)))
                row += w
            cnt_bytes = st["cnt"].contiguous().view(torch.uint8).view(nrec, 4)
            pairs.append((buf[:, nb_box + nb_sc + nb_feat:nb_box + nb_sc + nb_feat + 4], cnt_bytes))
            ops.copy_blocks(pairs)
            out = torch.empty((self.world * nrec, rec_bytes), dtype=torch.uint8, device=dev)
            self._count_wire("frame_records", buf)
            self.dist.all_gather_into_tensor(out, buf, group=self.group)
            c_all = out[:, nb_box + nb_sc + nb_feat:nb_box + nb_sc + nb_feat + 4].contiguous().view(torch.int32).view(-1)
            # my own frames keep their full records (views of this rank's frame-stage output)
            own_rows, row = {}, 0
            for slot, w in enumerate(mine_want):
                own_rows[slot] = (row, w)
                row += w
            order = []
            for pos, (r, slot) in enumerate(plan["place"]):
                g = r * nrec + slot
                if r == self.rank:
                    ro, w = own_rows[slot]
                    order.append((st["props"][slot, :w], st["scores"][slot, :w], st["feats"][ro:ro + w], c_all[g:g + 1], w))
                else:
                    rec = out[g]
                    order.append((rec[:nb_box].view(torch.float32).view(bn, 4), rec[nb_box:nb_box + bn * 4].view(torch.float32),
                                  rec[nb_box + nb_sc:nb_box + nb_sc + nb_feat].view(fdt).view(bn, D), c_all[g:g + 1], bn))
            g = {"recs": [o[:4] for o in order], "cnt": torch.cat([o[3] for o in order]), "want": [o[4] for o in order]}
            if "index" in st:
                g["index"] = {pos: st["index"][slot] for pos, (r, slot) in enumerate(plan["place"]) if r == self.rank}
            return {"gathered": g}
        # ---- legacy: whole records, one all-gather per row-count group
        got = {}
        row_off = 0
        for want, poss, per, first in plan:
            nb_box, nb_feat = want * 5 * 4, want * D * esz
            rec_bytes = (nb_box + nb_feat + 16 + 15) // 16 * 16
            buf = torch.zeros((per, rec_bytes), dtype=torch.uint8, device=dev)
            bs = torch.cat([st["props"][first:first + per, :want], st["scores"][first:first + per, :want, None]], dim=2)
            buf[:, :nb_box] = bs.contiguous().view(per, -1).view(torch.uint8)
            feats = st["feats"][row_off:row_off + per * want].reshape(per, want * D)
            buf[:, nb_box:nb_box + nb_feat] = feats.contiguous().view(torch.uint8)
            buf[:, nb_box + nb_feat:nb_box + nb_feat + 4] = st["cnt"][first:first + per].contiguous().view(per, 1).view(torch.uint8)
            row_off += per * want
            out = torch.empty((self.world * per, rec_bytes), dtype=torch.uint8, device=dev)
            self._count_wire("frame_records", buf)
            self.dist.all_gather_into_tensor(out, buf, group=self.group)
            bs_all = out[:, :nb_box].contiguous().view(torch.float32).view(-1, want, 5)
            f_all = out[:, nb_box:nb_box + nb_feat].contiguous().view(fdt).view(-1, want, D)
            c_all = out[:, nb_box + nb_feat:nb_box + nb_feat + 4].contiguous().view(torch.int32).view(-1)
            for slot, pos in enumerate(poss):
                got[pos] = (bs_all[slot, :, :4], bs_all[slot, :, 4], f_all[slot], c_all[slot:slot + 1])
        order = [got[p] for p in range(len(jobs))]
        g = {"recs": order, "cnt": torch.cat([r[3] for r in order]), "want": [int(j[1]) for j in jobs]}
        return {"gathered": g}

    @staticmethod
    def _cnt_of(h):
        return h["st"]["cnt"] if "st" in h else h["gathered"]["cnt"]

    def records_resolve(self, h, counts=None):
        """handle -> list of frame records.  counts: host list of the per-frame proposal counts (default: read
        them from the device, one host sync)."""
        if "st" in h:
            recs = self.model.frame_stage_resolve(h["st"], counts)
        else:
            g = h["gathered"]
            if counts is None:
                counts = g["cnt"].tolist()
            recs = []
            for i, w in enumerate(g["want"]):
                n = min(int(counts[i]), w)
                boxes, scores, feats, _ = g["recs"][i]
                recs.append({"boxes": boxes[:n], "scores": scores[:n], "feats": feats[:n]})
        if self.frame_model is not self.model:      # mixed-precision runs: the records enter the head in ITS stream dtype
            from .modeling import stream_dtype
            dt = stream_dtype(self.model.cfg)
            for r in recs:
                r["feats"] = r["feats"].to(dt)
        return recs

    def compute_records(self, clip, jobs):
        return self.records_resolve(self.records_async(clip, jobs))

    # ------------------------------------------------------------------ driver
    @torch.no_grad()
    def run(self, clip, T=None, gfor=None, first=0, last=None, on_step=None):
        """Process key frames first..last-1 of a T-frame video (first must be 0 for a fresh video, or the
        continuation of the previous call).  Returns the list of detections (BoxList, on device)."""
        m = self.model
        T = clip.shape[0] if T is None else T
        if gfor is None:
            gfor = global_schedule(T, m.cfg.MODEL.VID.MEGA.GLOBAL.SIZE)
        last = T if last is None else last
        H, W = (clip.shape[1], clip.shape[2]) if clip.dtype == torch.uint8 else (clip.shape[2], clip.shape[3])
        use_streams = clip.is_cuda and self.overlap
        sF = sB = cur = None
        if use_streams:
            if self._streams is None:
                # (a high-priority aggregation stream was measured in round 4: no effect on any block structure)
                self._streams = (torch.cuda.Stream(device=clip.device), torch.cuda.Stream(device=clip.device))
            sF, sB = self._streams
            cur = torch.cuda.current_stream(clip.device)
            sF.wait_stream(cur)
            sB.wait_stream(cur)
        batches = []
        idx = first
        if idx == 0 and idx < last:           # the cold start (13 local + GLOBAL.SIZE global frames) is its own batch
            batches.append((0, 1))
            idx = 1
        for n in self.batch_sizes(last - idx):
            batches.append((idx, idx + n))
            idx += n
        out = []
        pp = m.roi_heads.box.post_processor

        def prefetch(bi):      # host decodes of a later batch start while this one is being enqueued
            if hasattr(clip, "prefetch") and bi < len(batches):
                jobs = [j for i in range(*batches[bi]) for j in self.jobs_for_step(i, T, gfor)]
                if self.world > 1 and jobs:     # only this rank's slices of the frame stage (records_async's own plan)
                    jobs = [jobs[p] for p in self.shard_plan(jobs)[1]]
                clip.prefetch([j[0] for j in jobs])

        if first == 0:
            self._rec_cache, self._rec_pending = {}, set()

        # reuse_records: frames go through the frame stage in launches of EXACTLY frames_per_launch frames, taken in
        # the order in which the schedule first needs them (what a step-batch does not need yet is computed ahead of
        # time): one frame-stage shape for the whole video, i.e. one hipGraph, instead of a new shape per batch.
        plan, plan_pos = [], {}
        last_use = {}                     # reuse_records: frame id -> last key frame of this run() that consumes it
        if self.reuse_records:
            for i in range(first, last):
                for f, _, _ in self.jobs_for_step(i, T, gfor):
                    last_use[f] = i
                    if f not in plan_pos and f not in self._rec_cache and f not in self._rec_pending:
                        plan_pos[f] = len(plan)
                        plan.append(f)
        cursor = [0]

        def launch(flat):
            """one frame-stage launch (+ async copy of its proposal counts) -> handle"""
            early = {}

            def on_counts(c):     # between the two halves of the frame stage: counts -> pinned host memory + event
                if use_streams:
                    early["cnt_host"] = torch.empty(c.shape, dtype=c.dtype).pin_memory()
                    early["cnt_host"].copy_(c, non_blocking=True)
                    early["cnt_ev"] = torch.cuda.Event()
                    early["cnt_ev"].record(sF)
            h = self.records_async(clip, flat, on_counts if use_streams else None)
            h["jobs"] = flat
            h.update(early)
            if use_streams and "cnt_host" not in h:   # (sharded path: the counts arrive with the gathered records)
                c = self._cnt_of(h)
                h["cnt_host"] = torch.empty(c.shape, dtype=c.dtype).pin_memory()
                h["cnt_host"].copy_(c, non_blocking=True)
            return h

        def frame_stage(b):
            per_step = [self.jobs_for_step(i, T, gfor) for i in range(b[0], b[1])]
            flat = [j for js in per_step for j in js]
            launches = []
            if self.reuse_records:      # every frame once per video, always with the key-role row count
                need = [f for f, _, _ in flat if f not in self._rec_cache and f not in self._rec_pending]
                if need:
                    C = self.frames_per_launch
                    hi = max(plan_pos[f] for f in need) + 1
                    n = -(-(hi - cursor[0]) // C) * C
                    take = plan[cursor[0]:cursor[0] + n]
                    cursor[0] += len(take)
                    self._rec_pending.update(take)
                    take = take + [take[-1]] * (n - len(take))      # end of the plan: repeat (result ignored)
                    launches = [[(f, m.key_num, "l") for f in take[o:o + C]] for o in range(0, n, C)]
            else:
                if (self.use_graphs and clip.is_cuda and b[0] > 0 and 0 < b[1] - b[0] < self.steps_per_batch and per_step[-1]
                        and not self.ramp):
                    # a short last batch would be a NEW frame-stage shape: eager launches plus fresh allocator blocks
                    # (hipMalloc synchronises the device and stalls both streams, ~15 ms).  Pad it with repeats of
                    # its last step's jobs to the steady batch shape so that it replays the captured graph; the
                    # padded records are never consumed.
                    flat = flat + per_step[-1] * (self.steps_per_batch - (b[1] - b[0]))
                launches = [flat] if flat else []
            self.frames_computed += sum(len(x) for x in launches)
            if not launches:
                return per_step, [], None
            with _On(sF):
                hs = [launch(x) for x in launches]
                ev = None
                if use_streams:
                    ev = torch.cuda.Event()       # covers the launches and their count copies
                    ev.record(sF)
            return per_step, hs, ev

        def aggregate(b, per_step, hs, ev):
            with _On(sB):
                if use_streams and ev is not None:
                    sB.wait_event(ev)                 # GPU side: the aggregation starts after the whole frame stage
                    tw = _time.perf_counter()
                    # host side: only the proposal COUNTS are needed to lay the aggregation out; they were copied between
                    # the two halves of the frame stage, so the ~180 launches below are enqueued while res5 / ROIAlign /
                    # fc0 still run (a block of one step-batch used to spend 6 ms host-bound here after the GPU went idle)
                    for h in hs:
                        (h.get("cnt_ev") or ev).synchronize()
                    ht["frame_wait"] += _time.perf_counter() - tw
                recs = []
                for h in hs:
                    r = self.records_resolve(h, h["cnt_host"].tolist() if use_streams else None)
                    if self.reuse_records:
                        for (f, _, _), x in zip(h["jobs"], r):
                            self._rec_cache[f] = x
                            self._rec_pending.discard(f)
                    recs += r
                if use_streams:
                    for r in recs:                    # produced on sF, consumed on sB
                        for t in r.values():
                            t.record_stream(sB)
                pending, o = [], 0
                batched = (self.batch_aggregation and (self._static is None or not self.use_static)
                           and m.roi_heads.box.feature_extractor.cache_memory_kv)
                if self.owner_aligned and not batched and (self.world > 1 or self.force_sharded):
                    # owner-aligned dealing leaves non-owner ranks with base_num rows of a record: only the batched
                    # aggregation (one owner per key frame) can consume that; the per-frame path steps every key frame on
                    # every rank and would silently diverge (cache_memory_kv switched off after construction)
                    raise RuntimeError("ClipEngine: frames were dealt owner-aligned but the batched aggregation is off "
                                       "(cache_memory_kv / batch_aggregation changed after construction); build the engine "
                                       "after setting them")
                fe = m.roi_heads.box.feature_extractor
                # static mode: a key frame is its own batch of one step (whole records on every rank: never a shard)
                single = not batched and self._static is not None and fe.cache_memory_kv
                if not single and self._static is not None:
                    self._static.leave()          # the state goes back into the model's deques
                if not batched and self._sbatch is not None:
                    self._sbatch.leave()
                prepared = []                     # (key frame index, (new local record, new global records)) of
                                                  # the steps awaiting prepare_batch() + step_batch()

                def flush():
                    if not prepared:
                        return
                    shard = None
                    sharded = batched and (self.world > 1 or self.force_sharded)
                    if sharded and pp.candidates:
                        raise RuntimeError("ClipEngine: sharded key frames (KeyFrameShard) do not carry the candidates of "
                                           "TEST.BBOX_AUG / TEST.SOFT_NMS / TEST.BBOX_VOTE; run these with one rank per "
                                           "video (inference())")
                    if sharded:
                        # (legacy dealing: batch position t -> rank t mod world, whole records are everywhere)
                        shard = KeyFrameShard(self.dist, self.group_agg, self.rank, self.world,
                                              base=prepared[0][0] if self.owner_aligned else 0, wire=self.wire,
                                              order=self.wire_order)
                        self.wire_order.append("aggregate")
                    steps = [st for _, st in prepared]
                    # the owner of the fixed-address state this batch may run on: _static (a batch of one) or _sbatch
                    sb = None
                    if self.use_static and shard is None and prepared[0][0] > 0:
                        if single:
                            sb = self._static
                        elif self.graph_aggregation and clip.is_cuda and len(steps) == self.steps_per_batch:
                            if self._sbatch is None:
                                assert self._static is None
                                self._sbatch = StaticBatchAggregation(m, len(steps), keep_keys=self.keep_logits)
                            sb = self._sbatch
                    if sb is not None and sb.ready(steps):
                        c0 = sb.captures
                        outs, frames = sb.step(steps, (W, H))
                        if single:
                            self.static_steps += 1
                        else:
                            self.graph_stats["agg_captured"] = self.graph_stats.get("agg_captured", 0) + sb.captures - c0
                            self.graph_stats["agg_replayed"] = sb.replays
                    else:
                        for owner in (self._static, self._sbatch):
                            if owner is not None:
                                owner.leave()
                        frames = m.prepare_batch(steps)
                        outs = m.step_batch(frames, (W, H), shard)
                    for (i2, _), pd in zip(prepared, outs):
                        pending.append((i2, pd))
                    if self.keep_logits:     # (sharded: only this rank's own key frames have logits here)
                        self.logits_log += [None if x is None else x.float().clone() for x in m.last_logits_batch]
                        self.key_boxes_log += [f["rois_key"].clone() for f in frames]
                        self.key_index_log += [None if f.get("index_key") is None else f["index_key"].clone() for f in frames]
                    del prepared[:]

                for i, js in zip(range(b[0], b[1]), per_step):
                    if self.reuse_records:
                        r = [self._rec_cache[j[0]] for j in js]
                        if last == T:         # whole video scheduled: a record is dropped after its last use (a
                            for j in js:      # multi-thousand-frame video would otherwise keep ~1 MB per frame)
                                if last_use.get(j[0]) == i:
                                    self._rec_cache.pop(j[0], None)
                    else:
                        r = recs[o:o + len(js)]
                        o += len(js)
                    loc = [x for x, j in zip(r, js) if j[2] == "l"]
                    glob = [x for x, j in zip(r, js) if j[2] == "g"]
                    new_local = loc[0]
                    if i == 0:
                        if self._static is not None:
                            self._static.reset()
                        if self._sbatch is not None:
                            self._sbatch.reset()
                        m._reset(T)
                        for _ in range(m.key_frame_location + 1):
                            m.records.append(loc[0])
                        for x in loc[1:]:
                            m.records.append(x)
                        new_local = None
                    if batched:
                        prepared.append((i, (new_local, glob)))
                    elif single and i > 0:
                        prepared.append((i, (new_local, glob)))
                        flush()
                    else:                     # the cold start of the per-frame lanes; no batched path (RDN, cache_memory_kv off)
                        pending.append((i, m.step(new_local, glob, (W, H), defer=True)))
                        if self.keep_logits:
                            key = m.records[m.key_frame_location]
                            self.logits_log.append(m.last_logits.float().clone())
                            self.key_boxes_log.append(key["boxes"].clone())
                            self.key_index_log.append(key["index"].clone() if "index" in key else None)
                flush()
                if use_streams:   # detection counts of the whole batch -> pinned host memory, async + event
                    dc = torch.cat([pd[3] for _, pd in pending])
                    host = torch.empty(dc.shape, dtype=dc.dtype).pin_memory()
                    host.copy_(dc, non_blocking=True)
                    evb = torch.cuda.Event()
                    evb.record(sB)
                    pending.append((host, evb))
            return pending

        def finish(pending):
            # one host read per batch of steps: all detection counts, then cut the padded outputs
            if use_streams:
                host, evb = pending.pop()
                evb.synchronize()                     # waits for this batch's aggregation only
                counts = host.tolist()
            else:
                counts = torch.cat([pd[3] for _, pd in pending]).tolist()
            for (i, pd), n in zip(pending, counts):
                if int(n) > pd[0].shape[0]:
                    raise RuntimeError("key frame %d: %d detections but only %d rows travelled (KeyFrameShard cap)"
                                       % (i, int(n), pd[0].shape[0]))
                det = pp.materialize(pd, int(n), (W, H))
                out.append(det)
                if on_step is not None:
                    on_step(i, det)

        import time as _time
        ht = self.host_times
        prefetch(0)
        prefetch(1)
        staged = frame_stage(batches[0]) if batches else None
        if hasattr(clip, "stage_ahead") and last < T and self.world == 1 and not self.reuse_records and batches:
            # read-ahead across calls: the step-batch that FOLLOWS this range is staged (host copies + H2D on the source's own
            # stream) while this range's frame stage / aggregation run -- a caller that walks the video block by block (the
            # benchmark's with-H2D leg, inference.py's loop) never waits for a batch's 72 MB at the top of its block
            nb = (last, min(T, last + self.steps_per_batch))
            clip.stage_ahead([j[0] for i in range(*nb) for j in self.jobs_for_step(i, T, gfor)])
        prev_pending = None
        for bi, b in enumerate(batches):
            t0 = _time.perf_counter()
            prefetch(bi + 2)
            nxt = frame_stage(batches[bi + 1]) if bi + 1 < len(batches) else None   # F(b+1): async, enqueued first
            t1 = _time.perf_counter()
            pending = aggregate(b, *staged)                                        # B(b): runs beside F(b+1)
            t2 = _time.perf_counter()
            if prev_pending is not None:
                finish(prev_pending)                                               # results of B(b-1)
            t3 = _time.perf_counter()
            ht["frame_enqueue"] += t1 - t0
            ht["aggregate_enqueue"] += t2 - t1      # (includes frame_wait)
            ht["finish_wait"] += t3 - t2
            ht["steps"] += b[1] - b[0]
            prev_pending, staged = pending, nxt
        if prev_pending is not None:
            finish(prev_pending)
        if use_streams:
            cur.wait_stream(sF)
            cur.wait_stream(sB)
        return out


class StaticBatchAggregation(object):
    """The BATCHED aggregation of a step-batch (GeneralizedRCNNMEGA.prepare_batch + step_batch: tapes, 7 batched attention
    stages, stage FCs, predictor, post-processing of S key frames; ~100 launches and ~6 ms of Python per 20 key frames) on
    FIXED-ADDRESS state, captured once as a hipGraph and replayed with one host call per step-batch.

    A driver-CLI block is one frame-stage batch followed by its aggregation: the aggregation's kernels are short, so the
    host could not keep the queue full (0.5 ms of gaps per 22.5 ms block in round 3, more with the f32 head stream's extra
    launches) -- a replay has none.

    Steady state = the local window, the global pool and all memory pools are full and every record involved has all its
    proposals: every tensor of the batch then has a fixed shape.  The per-video state (last 25 frame records, global
    pool, memory pools with their cached K / V^T projections) lives in state tensors; a step copies the S new records into
    input buffers (one launch), runs / replays the UNCHANGED prepare_batch + step_batch on deques that are views of the
    state, and -- inside the captured region -- writes the state the batch leaves behind back into the state tensors.  The
    kernels and their operand values are those of the eager path: identical bits (tests/test_e2e_gpu.py::
    test_graph_aggregation_is_bit_identical; the host logic on the CPU twins in tests/test_host_logic.py).
    Anything else (a ragged record, a short last batch, a new video, sharding) leaves: the state goes back into the
    model's own deques and the eager path continues.

    S = 1 is the per-key-frame lane (ClipEngine(static_aggregation=True), bench.py --aggregation static): one replay per
    key frame.  While active, an instance owns the model's per-video state, so a model has at most one active instance:
    ClipEngine holds either _static (S = 1) or _sbatch (S = steps_per_batch), never both.
    keep_keys: the key frames' boxes / anchor indices in the returned frames are copies (an engine that logs them), not
    views of state that the write-back has already shifted."""

    def __init__(self, model, S, use_graph=True, keep_keys=False):
        self.m = model
        self.fe = model.roi_heads.box.feature_extractor
        self.S = S
        self.use_graph = use_graph
        self.keep_keys = keep_keys
        self.active = False
        self.graph = None
        self.replays = 0
        self.captures = 0

    # ---- conditions
    def ready(self, steps):
        m, fe = self.m, self.fe
        if not (m.memory_enable and m.global_enable and fe.cache_memory_kv):
            return False
        if len(steps) != self.S:
            return False
        for new_local, new_globals in steps:
            if new_local is None or len(new_globals) != 1 or new_local["boxes"].shape[0] != m.key_num:
                return False
            if new_globals[0]["feats"].shape[0] < m.base_num:
                return False
        if self.active:
            return True
        if len(m.records) != m.all_frame_interval or any(r["boxes"].shape[0] != m.key_num for r in m.records):
            return False
        gq = fe.global_queue_list[0]["feats"]
        if len(gq) != fe.global_size or any(g.shape[0] != m.base_num for g in gq):
            return False
        for i in range(fe.stage):
            q = fe.mem_queue_list[i]
            n = m.base_num if i == 0 else m.advanced_num
            if len(q["k"]) != fe.all_frame_interval or len(q["rois"]) != fe.all_frame_interval:
                return False
            if any(t.shape[0] != n for t in q["rois"]):
                return False
        return True

    # ---- eager state -> state tensors
    def enter(self, steps):
        m, fe, S = self.m, self.fe, self.S
        recs = list(m.records)
        self.keys = [k for k in ("boxes", "scores", "feats", "index") if all(k in r for r in recs) and
                     all(k in st[0] for st in steps)]
        self.hist = {k: torch.stack([r[k] for r in recs]).contiguous() for k in self.keys}      # [25, 300, ...] oldest first
        self.glob = torch.cat(list(fe.global_queue_list[0]["feats"]), dim=0).contiguous()
        self.mem = [{"rois": torch.cat(list(fe.mem_queue_list[i]["rois"]), 0).contiguous(),
                     "k": torch.cat(list(fe.mem_queue_list[i]["k"]), 0).contiguous(),
                     "vt": torch.cat(list(fe.mem_queue_list[i]["vt"]), 1).contiguous()} for i in range(fe.stage)]
        self.inp = {k: torch.zeros((S,) + tuple(self.hist[k].shape[1:]), dtype=self.hist[k].dtype, device=self.hist[k].device)
                    for k in self.keys}
        self.in_glob = torch.zeros((S, m.base_num, self.glob.shape[1]), dtype=self.glob.dtype, device=self.glob.device)
        self.active = True
        self.graph = None
        self._rebind()

    def _rebind(self):
        """the model's deques / caches as views of the state tensors (the configuration the graph was captured in)"""
        m, fe = self.m, self.fe
        n25 = m.all_frame_interval
        m.records = deque(({k: self.hist[k][f] for k in self.keys} for f in range(n25)), maxlen=n25)
        gq = fe.global_queue_list[0]["feats"]
        gq.clear()
        bn = m.base_num
        for j in range(fe.global_size):
            gq.append(self.glob[j * bn:(j + 1) * bn])
        fe.global_cache[0]["feats"] = self.glob
        for i in range(fe.stage):
            n = m.base_num if i == 0 else m.advanced_num
            q = fe.mem_queue_list[i]
            for key in ("rois", "k", "vt"):
                q[key].clear()
            for f in range(fe.all_frame_interval):
                q["rois"].append(self.mem[i]["rois"][f * n:(f + 1) * n])
                q["k"].append(self.mem[i]["k"][f * n:(f + 1) * n])
                q["vt"].append(self.mem[i]["vt"][:, f * n:(f + 1) * n])
            fe.mem[i] = dict(self.mem[i])

    # ---- state tensors -> eager state (leaving steady state)
    def leave(self):
        if not self.active:
            return
        m, fe = self.m, self.fe
        self._rebind()
        m.records = deque(({k: v.clone() for k, v in r.items()} for r in m.records), maxlen=m.records.maxlen)
        gq = fe.global_queue_list[0]["feats"]
        gl = [g.clone() for g in gq]
        gq.clear()
        for g in gl:
            gq.append(g)
        fe.global_cache[0]["feats"] = torch.cat(gl, dim=0)
        for i in range(fe.stage):
            q = fe.mem_queue_list[i]
            for key in ("rois", "k", "vt"):
                items = [t.clone() for t in q[key]]
                q[key].clear()
                for t in items:
                    q[key].append(t)
            fe.mem[i] = {"rois": torch.cat(list(q["rois"]), 0), "k": torch.cat(list(q["k"]), 0),
                         "vt": torch.cat(list(q["vt"]), 1)}
        self.active = False
        self.graph = None

    def reset(self):
        """new video: the model re-creates its deques; drop the static state without writing it back"""
        self.active = False
        self.graph = None

    # ---- one step-batch on the static state (this body is what the graph captures)
    def _body(self, im_size):
        m, fe, S = self.m, self.fe, self.S
        steps = [({k: self.inp[k][t] for k in self.keys}, [{"feats": self.in_glob[t]}]) for t in range(S)]
        frames = m.prepare_batch(steps)
        outs = m.step_batch(frames, im_size)
        if self.keep_keys:
            for f in frames:
                f["rois_key"] = f["rois_key"].clone()
                f["index_key"] = None if f["index_key"] is None else f["index_key"].clone()
        # the state the batch leaves behind -> the state tensors, through temporaries (sources may be views of the state)
        groups = [([r[k].reshape(r[k].shape[0], -1) for r in m.records], 0) for k in self.keys]
        tmp = ops.multi_cat(groups)
        pairs = [(self.hist[k].view(tmp[j].shape), tmp[j]) for j, k in enumerate(self.keys)]
        pairs.append((self.glob, fe.global_cache[0]["feats"]))
        for i in range(fe.stage):
            for key in ("rois", "k", "vt"):
                pairs.append((self.mem[i][key], fe.mem[i][key]))
        # (global pool / memory pools: their new contents are tapes of this batch, never views of the state tensors)
        ops.copy_blocks(pairs)
        # the S padded outputs as four tensors: a replay hands out 4 clones, not 4 S
        packed = tuple(torch.stack([o[j] for o in outs]) for j in range(4))
        return packed, frames

    @staticmethod
    def _unpack(packed, clone):
        ob, os_, ol, oc = (t.clone() for t in packed) if clone else packed
        return [(ob[t], os_[t], ol[t], oc[t]) for t in range(ob.shape[0])]

    @torch.no_grad()
    def step(self, steps, im_size):
        """steps = [(new local record, [new global record])] x S -> (padded post-processing outputs of the S key frames,
        the frames list of prepare_batch: rois_key etc. for logging)."""
        if not self.active:
            self.enter(steps)
        pairs = []
        for t, (loc, globs) in enumerate(steps):
            for k in self.keys:
                pairs.append((self.inp[k][t].reshape(loc[k].shape[0], -1), loc[k].reshape(loc[k].shape[0], -1)))
            pairs.append((self.in_glob[t], globs[0]["feats"][:self.m.base_num]))
        ops.copy_blocks(pairs)
        if not (self.use_graph and self.glob.is_cuda) or self.graph is None:
            # no graphs (CPU twins) / the first steady batch: eager on the static state (warms every host-side cache --
            # index tables, zero pads, packed weights -- before the capture)
            if self.use_graph and self.glob.is_cuda:
                self.graph = "armed"
            packed, frames = self._body(im_size)
            self._rebind()
            return self._unpack(packed, False), frames
        if self.graph == "armed":                   # second steady batch: capture
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):      # (see ClipEngine._frame_stage)
                self._out = self._body(im_size)
            self._rebind()
            self.graph = g
            self.captures += 1
        self.graph.replay()
        self.replays += 1
        packed, frames = self._out
        return self._unpack(packed, True), frames

