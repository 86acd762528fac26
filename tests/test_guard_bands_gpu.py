"""-m gpu: no kernel writes outside its output, its workspace or a caller's destination.

tests/test_stale_memory_gpu.py shows that no result depends on bytes the kernel did not write; this file is the mirror image.
A kernel that writes bytes it does not own -- a 16-byte store over a 6-byte tail, an unmasked last tile row, a workspace the C
ABI sized one row short, a pad-key column past Nk -- passes every test that only compares the tensor it asked for: the stray
bytes land in the allocator's round-up padding or in a neighbour.  poison.guarded() carves every allocation of the modules
under test (torch.empty / empty_like / zeros / zeros_like / full and ops._ws) from one slab, each between two guard bands that
start at the payload's exact first and last byte, and p.check() reports every band byte that changed.

Each case asserts three things, under both polarities ("ff": bands 0x00 / payload 0xFF, "00": bands 0xFF / payload 0x00 -- a
stray byte differs from one of the two patterns):

  1. p.check() passes: every band of every allocation holds its pattern, and every input placed with p.place() still holds
     what was placed (except the documented in-place destinations registered with p.writes());
  2. the defined outputs are bit-equal between the two polarities and to a clean, unguarded run;
  3. the case's own reference check passes (on the clean run: 2. makes the three runs the same bits).

Bit-equality across the polarities also shows that no result depends on what lies beyond an input's last byte: beyond a
placed input there is 0x00 under one polarity and 0xFF under the other.  It CANNOT show a masked out-of-range load -- a load
past the end whose value is discarded changes nothing here -- and nothing in this file passes a kernel a buffer smaller than
it is told.  Operands of 2 GiB or more and graph captures are out of scope (the fills and checks are extra launches).

Part A fences every case of the stale-memory table (its run / check functions, inputs where its builders put them).
Part B runs tail shapes -- the smallest at which a store can overrun -- with the inputs placed, so that every operand ends
exactly where a band begins.  The conv family's bands are at least rows x ldo x element size wide, rows asked from
mega_conv2d_nhwc_plan_ex, so that a whole stray tile lands in the band and not behind it; everything else uses 64 KiB.

GUARD_OPS names, for every function of ops.py whose source contains a _call(, the tests below that run it fenced;
tests/test_guard_bands.py (CPU) fails when a launching wrapper has no entry."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import box_boundary_cases as bc
import cpu_ops
import diagnose_cases
import diagnose_twin
import exact_conv_cases as ec
import f8_conv_cases as fc
import jpeg_cases
import motion_iou_cases
import motion_iou_twin
import multi_launch_cases as mc
import overlay_twin
import poison
import sampling_lattice_cases as sc
import seq_nms_cases
import seq_nms_twin
import test_stale_memory_gpu as sm
from test_track_refine import assert_frames_equal
import track_eval_cases
import track_eval_twin
import track_refine_cases
import track_refine_twin
import tracks_cases
import tracks_twin
import vid_twin
from oracle import native

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
_NAME = {BF16: "bf16", F16: "f16", F32: "f32"}
GUARD = 65536
SLAB_B = 48 << 20                      # Part B: one slab size for every tail shape (the largest case uses a few MiB)
POLARITIES = ("ff", "00")

# function of ops.py that launches a kernel -> the tests below that run it fenced
GUARD_OPS = {
    "conv2d_nhwc": ("test_gemm_table", "test_conv_tile_tails", "test_conv_geometry_and_split_k"),
    "_conv1x1_strided_residual": ("test_gemm_table", "test_conv_geometry_and_split_k"),
    "deconv4x4s2_into": ("test_gemm_table", "test_deconv_into_a_wider_buffer"),
    "conv2d_sp": ("test_gemm_table", "test_conv2d_sp_tails"),
    "conv2d_nhwc_f8": "test_conv_f8_tails",
    "linear_transposed": ("test_gemm_table", "test_linear_transposed_tails"),
    "linear_transposed_x3": ("test_gemm_table", "test_linear_transposed_tails"),
    "flow_conv1_combine": ("test_fgfa_flownet_table", "test_flow_tails"),
    "flow_pred_finish": ("test_fgfa_flownet_table", "test_flow_tails"),
    "flow_level_assemble": ("test_fgfa_flownet_table", "test_flow_tails"),
    "dff_warp_scale": ("test_fgfa_flownet_table", "test_flow_tails"),
    "fgfa_warp_aggregate": ("test_fgfa_flownet_table", "test_fgfa_tails"),
    "fgfa_warp_aggregate_group": ("test_fgfa_flownet_table", "test_fgfa_tails"),
    "fgfa_pair_taps": ("test_fgfa_flownet_table", "test_fgfa_tails"),
    "bottleneck64": ("test_spatial_table", "test_bottleneck_tails"),
    "bottleneck64_ds": ("test_spatial_table", "test_bottleneck_tails"),
    "stem": "test_stem_tails",
    "stem_u8": "test_stem_tails",
    "stem_pool": ("test_spatial_table", "test_stem_tails"),
    "maxpool3x3s2": ("test_spatial_table", "test_pool_tails"),
    "avgpool2x2_ceil": ("test_spatial_table", "test_pool_tails"),
    "roi_align": ("test_spatial_table", "test_roi_align_tails"),
    "roi_align_planes": ("test_spatial_table", "test_roi_align_tails"),
    "nms": ("test_nms_table", "test_nms_tails"),
    "rpn_select": ("test_rpn_select_table", "test_rpn_select_tails"),
    "postprocess": ("test_postprocess_table", "test_postprocess_tails"),
    "postprocess_batched": ("test_postprocess_table", "test_postprocess_tails"),
    "postprocess_candidates_batched": ("test_postprocess_table", "test_postprocess_tails"),
    "bbox_aug_merge": ("test_merge_table", "test_merge_tails"),
    "soft_merge": ("test_merge_table", "test_merge_tails"),
    "position_logits": ("test_attention_table", "test_position_logits_tails"),
    "position_logits_batched": ("test_attention_table", "test_position_logits_tails"),
    "relation_attention_batched": ("test_attention_table", "test_attention_tails"),
    "copy_blocks": ("test_copies_casts_table", "test_copy_tails"),
    "cat_rows_cast_bf16": ("test_copies_casts_table", "test_copy_tails"),
    "cast_half": ("test_copies_casts_table", "test_cast_tails"),
    "split_bf16x3": ("test_copies_casts_table", "test_cast_tails"),
    "split_planes": ("test_copies_casts_table", "test_cast_tails"),
    "resize_bilinear_u8": ("test_spatial_table", "test_resize_tails"),
    "resize_bilinear_u8_flip": ("test_spatial_table", "test_resize_tails"),
    "preprocess_frames": "test_preprocess_frames_tails",
    "jpeg_reconstruct": "test_jpeg_reconstruct_tails",
    "overlay_detections": ("test_evaluation_table", "test_overlay_tails"),
    "vid_eval_match": ("test_evaluation_table", "test_evaluation_hand_sets"),
    "vid_eval_ap": ("test_evaluation_table", "test_evaluation_hand_sets"),
    "proposal_recall_match": "test_evaluation_table",
    "seq_nms": ("test_evaluation_table", "test_evaluation_hand_sets"),
    "link_tracks": ("test_evaluation_table", "test_evaluation_hand_sets"),
    "refine_tracks": "test_refine_tracks",
    "tubelet_scores": ("test_evaluation_table", "test_evaluation_hand_sets"),
    "tubelet_match": ("test_evaluation_table", "test_evaluation_hand_sets"),
    "motion_iou": ("test_evaluation_table", "test_evaluation_hand_sets"),
    "diagnose_match": "test_diagnose",
}
# every module some case fences (the CPU file reads their source for allocation idioms the proxy cannot see)
MODULE_NAMES = tuple(sm.MODULE_NAMES) + ("diagnose",)
EVAL_MODULES = ("ops", "seq_nms", "tracks", "track_eval", "vid_eval", "motion_iou", "diagnose", "flat")

_mods, _ops, _lib, _host, _same = sm._mods, sm._ops, sm._lib, sm._host, sm._same


# ===================================================================================================== the harness
def _check_kept(kept, polarity, what):
    """a region the wrapper leaves alone on purpose (sm's "untouched") still holds the payload's pre-fill"""
    fill = poison.POLARITIES[polarity][1]
    for k, v in kept.items():
        raw = np.frombuffer(sm._bytes(v), np.uint8)
        assert raw.size and (raw == fill).all(), "%s under %s: %s was written (%d of %d bytes)" % (
            what, polarity, k, int((raw != fill).sum()), raw.size)


_NEED = {}


def _table(case, dev, guard_bytes=GUARD):
    """Part A: one case of the stale-memory table, fenced.  The slab: a dry `ones` run's p.nbytes plus 2 x guard_bytes + 512
    per counted allocation (and room for the few zeros / full allocations the dry run's helper does not count)."""
    want = sm._clean(case, dev)                                            # two clean runs bit-equal + the reference check
    modules = case.modules or _mods("ops")
    if case.name not in _NEED:
        with poison.poisoned("ones", modules) as dry:
            sm._snap(case, "B", dev)
        _NEED[case.name] = dry.nbytes + (dry.count + 24) * (2 * guard_bytes + 512) + (1 << 20)
    for polarity in POLARITIES:
        with poison.guarded(modules, slab_bytes=_NEED[case.name], device=dev, guard_bytes=guard_bytes, polarity=polarity) as p:
            out = case.run("B", dev)
            torch.cuda.synchronize()
            p.check()
            kept = out.pop("untouched", {}) if isinstance(out, dict) else {}
            got, kept = _host(out), _host(kept)
        assert p.count >= 1, "%s: no allocation went through the helper" % case.name
        _same(got, want, "%s fenced, polarity %s" % (case.name, polarity))
        _check_kept(kept, polarity, case.name)
        if case.check is not None and polarity == "ff":                    # (the same bits as the clean run: once is enough)
            case.check(got)


def _fenced(fn, dev, what, modules=None, guard_bytes=GUARD, slab_bytes=SLAB_B, own=1):
    """Part B: fn(put, writes) -> outputs.  put(t) brings a host tensor to the device -- .to(dev) in the clean run, p.place in
    the fenced ones, so that the operand ends where a band begins; writes(t) registers a placed tensor as an in-place
    destination.  own: the least number of allocations the code under test makes itself (0 where it writes only into the
    caller's destination, or launches nothing).  -> the clean run's outputs on the host, for the caller's reference check."""
    modules = modules or _mods("ops")
    clean = fn(lambda t: t.to(dev), lambda t: t)
    torch.cuda.synchronize()
    clean = _host(clean)
    for polarity in POLARITIES:
        with poison.guarded(modules, slab_bytes=slab_bytes, device=dev, guard_bytes=max(GUARD, guard_bytes), polarity=polarity) as p:
            out = fn(p.place, p.writes)
            torch.cuda.synchronize()
            p.check()
            got, npl = _host(out), len(p.placed)
        assert p.count - npl >= own, "%s: no allocation of the wrapper went through the helper" % what
        _same(got, clean, "%s fenced, polarity %s" % (what, polarity))
    return clean


def _np(put, a):
    return put(torch.from_numpy(np.ascontiguousarray(a)))


def test_the_device_path_of_the_helper_catches_a_planted_byte(dev):
    """tests/test_guard_bands.py proves the helper on CPU tensors; this is its device path (the stacked reduction, the read-back
    on a mismatch).  The fault is a plain tensor write through the slab's uint8 view: no kernel is asked to misbehave."""
    ops = _ops()
    seen = {}
    for polarity in POLARITIES:
        with poison.guarded((ops,), slab_bytes=1 << 20, device=dev, guard_bytes=4096, polarity=polarity) as p:
            x = p.place(torch.arange(75, dtype=torch.int16))
            y = ops.cast_half(p.place(torch.ones(75)), BF16)               # 150 bytes: ends on no 16-byte boundary
            w = ops._ws(4950, dev)
            torch.cuda.synchronize()
            p.check()
            at = y.data_ptr() - p.slab.data_ptr()
            assert at % poison.ALIGN == 0 and p.allocs[2].kind == "empty" and "ops.py" in p.allocs[2].site
            p.slab[at + 150:at + 160] = 0xFF                               # a 16-byte store over a 6-byte tail
            p.slab[w.data_ptr() - p.slab.data_ptr() - 1] = 0xFF
            x[3] = 7
            torch.cuda.synchronize()
            try:
                p.check()
                seen[polarity] = ""
            except AssertionError as e:
                seen[polarity] = str(e)
    # 0xFF is the "00" polarity's own band pattern: only the placed input shows there; "ff" sees all three
    assert "allocation #2 (empty, shape (75,), bfloat16, 150 bytes)" in seen["ff"] and "first at offset +0 and last at +9" in seen["ff"]
    assert "allocation #3 (_ws, shape (4950,), uint8, 4950 bytes)" in seen["ff"] and "first at offset -1 and last at -1" in seen["ff"]
    for polarity in POLARITIES:
        assert "allocation #0 (placed, shape (75,), int16, 150 bytes)" in seen[polarity] and "first at offset 6 and last at 6" in seen[polarity]
    assert "band overwritten" not in seen["00"]


# ===================================================================================================== Part A: the stale table
@pytest.mark.parametrize("n", sm.NMS_N)
def test_nms_table(dev, n):
    _table(sm._NMS()["nms-%d" % n], dev)


@pytest.mark.parametrize("form", sorted(sm.RPN_STALE))
def test_rpn_select_table(dev, form):
    _table(sm._RPN()["rpn-" + form], dev)


@pytest.mark.parametrize("op", ["postprocess", "postprocess_batched", "postprocess_candidates_batched"])
def test_postprocess_table(dev, op):
    _table(sm._POST()[op], dev)


@pytest.mark.parametrize("op", sorted(sm.MERGE_KW))
def test_merge_table(dev, op):
    _table(sm._MERGE()[op], dev)


@pytest.mark.parametrize("name", sm.GEMM_NAMES)
def test_gemm_table(dev, name, monkeypatch):
    """(bands of 1 MiB: a 256-row tile of the widest case here, 264 f32 columns, is 270 KB)"""
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    _table(sm._GEMM()[name], dev, guard_bytes=1 << 20)


@pytest.mark.parametrize("name", ["attention-chain-bf16", "attention-chain-f32", "position_logits"])
def test_attention_table(dev, name):
    _table(sm._ATTN()[name], dev)


@pytest.mark.parametrize("name", sm.FLOW_NAMES)
def test_fgfa_flownet_table(dev, name):
    _table(sm._FLOW()[name], dev, guard_bytes=(1 << 20) if name.startswith("flow-level") else GUARD)


@pytest.mark.parametrize("name", sm.SPATIAL_NAMES)
def test_spatial_table(dev, name):
    _table(sm._SPATIAL()[name], dev)


@pytest.mark.parametrize("name", ["copy_blocks-multi_cat", "casts"])
def test_copies_casts_table(dev, name):
    _table(sm._COPY()[name], dev)


@pytest.mark.parametrize("name", sm.EVAL_NAMES)
def test_evaluation_table(dev, name):
    _table(sm._EVAL()[name], dev)


def test_whole_model_eager_fenced(dev):
    """The small synthetic R-50 MEGA clip of test_e2e_gpu.py (bf16, eager, no graph capture) with every allocation of ops,
    modeling, relation, rdn and engine between 4 KiB bands: detections and logits bit-equal to the clean run under both
    polarities, no band touched."""
    modules = _mods("ops", "modeling", "relation", "rdn", "engine")
    clean = _host(sm._mega_run(dev, "bfloat16"))
    assert sum(len(d[1]) for d in clean["dets"]) > 0
    with poison.poisoned("ones", modules) as dry:
        sm._mega_run(dev, "bfloat16")
    need = dry.nbytes + (dry.count + 256) * (2 * 4096 + 512) + (8 << 20)
    for polarity in POLARITIES:
        with poison.guarded(modules, slab_bytes=need, device=dev, guard_bytes=4096, polarity=polarity) as p:
            got = sm._mega_run(dev, "bfloat16")
            torch.cuda.synchronize()
            p.check()
            got = _host(got)
        assert p.count >= 1 and p.ws_count >= 1
        _same(got, clean, "MEGA bf16 fenced, polarity %s" % polarity)


# ===================================================================================================== Part B: conv / linear
TILES = ["natural", "64x64", "128x64", "128x128", "256x128", "256x256", "8:256", "8:192"]


def _plan(shape, dtype, odt, has_res=False, ldo=None):
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    ops = _ops()
    t = _lib().mega_conv2d_nhwc_plan_ex(N, H, W, Cin, Cout, R, R, stride, pad, dil, ldo or Cout, int(has_res), ops._DT[dtype],
                                        ops._DT[odt])
    return t // 1000000, t % 1000000 // 1000, t % 1000


def _esize(dtype):
    return 4 if dtype == F32 else 2


def _conv_fn(case, **kw):
    N, H, W, Cin, Cout, R, stride, pad, dil = case.shape

    def fn(put, writes):
        return {"y": _ops().conv2d_nhwc(put(case.x), put(case.w), put(case.scale), put(case.bias),
                                        None if case.res is None else put(case.res), stride=stride, pad=pad, dil=dil,
                                        relu=case.relu, out_dtype=case.out_dtype, **kw)}
    return fn


def _conv_guard(shape, dtype, odt, has_res=False):
    """rows x ldo x element size of the tile the launch path's own rule gives this layer (f32 partial sums: 4 bytes)"""
    kind, rows, cols = _plan(shape, dtype, odt, has_res)
    return rows * shape[4] * 4, (kind, rows, cols)


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("tile", TILES)
def test_conv_tile_tails(dev, tile, dtype, monkeypatch):
    """For the tile the dispatch returns -- naturally, and under each value of the library's own tile switch -- a 1x1 conv with
    M = rows + 1 and M = 1 rows and Cout = cols + 8 and Cout = 8 columns, rows x cols asked from mega_conv2d_nhwc_plan_ex:
    one row and eight columns past a full tile, and far less than one."""
    if tile == "natural":
        monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    else:
        monkeypatch.setenv("MEGA_IGEMM_TILE", tile)
    _, rows, cols = _plan((1, 1, 300, 64, 264, 1, 1, 0, 1), dtype, dtype)
    assert rows in (64, 128, 192, 256) and cols in (64, 128, 256)
    if tile not in ("natural",) and not (tile.startswith("8:") and dtype == F32):
        want = (int(tile[2:]), 256) if tile.startswith("8:") else tuple(int(v) for v in tile.split("x"))
        assert (rows, cols) == want, "the switch %s gave tile %d x %d" % (tile, rows, cols)
    # K = 64; under the igemm8 switches also K = 576 > 512: the matrix class (8) next to the streaming class (7)
    for K in (64, 576) if (tile.startswith("8:") and dtype != F32) else (64,):
        for M in (rows + 1, 1):
            for Cout in (cols + 8, 8):
                shape = (1, 1, M, K, Cout, 1, 1, 0, 1)
                guard, plan = _conv_guard(shape, dtype, dtype, True)
                if tile.startswith("8:") and dtype != F32:
                    assert plan == (7 if K <= 512 else 8, int(tile[2:]), 256), (shape, plan)
                case = ec.make_case(shape, dtype, dtype, 1, True, seed=M + Cout + K)
                what = "conv 1x1 M %d Cout %d K %d %s tile %s (plan %s)" % (M, Cout, K, _NAME[dtype], tile, plan)
                got = _fenced(_conv_fn(case), dev, what, guard_bytes=guard)
                ec.assert_bits_equal(got["y"], ec.reference(case)[0], what, relu=1, tile=plan[1:])


CONV_GEOMETRY = [("3x3-pad1-5x7", (1, 5, 7, 64, 72, 3, 1, 1, 1)), ("3x3-stride2-13x15", (1, 13, 15, 64, 72, 3, 2, 1, 1)),
                 ("lib-splitk", sm.LIB_SPLITK), ("ksplit4", ec.CALLER_SPLITK_SHAPE), ("ksplit1000", ec.CALLER_SPLITK_SHAPE),
                 ("strided-residual", sm.RS_SHAPE), ("conv64", ec.CONV64_SHAPE)]
# (the strided-residual launch and the 64-channel 3x3 kernel take 16-bit tensors only)
CONV_GEOMETRY_CASES = [(n, s, dt) for n, s in CONV_GEOMETRY for dt in (BF16, F16, F32)
                       if not (dt == F32 and n in ("strided-residual", "conv64"))]


@pytest.mark.parametrize("name,shape,dtype", CONV_GEOMETRY_CASES, ids=["%s-%s" % (n, _NAME[dt]) for n, _, dt in CONV_GEOMETRY_CASES])
def test_conv_geometry_and_split_k(dev, name, shape, dtype, monkeypatch):
    """3x3 / pad 1 on 5 x 7 (35 rows), 3x3 / stride 2 on 13 x 15 (7 x 8 outputs); split-K by the library's rule with the
    workspace of exactly mega_conv2d_nhwc_workspace_bytes, the caller's ksplit 4 and 1000 (clamped) with exactly
    mega_conv2d_nhwc_ks_workspace_bytes (the wrapper asks for that many bytes and the band starts behind the last one);
    _conv1x1_strided_residual reading the 9 x 13 residual in place; the 64-channel 3x3 kernel (launch class 6, which the
    dispatch gives only to a large map) on 5 x 70 x 90 = 31500 rows, no multiple of its 256-row tile."""
    monkeypatch.delenv("MEGA_IGEMM_TILE", raising=False)
    ops, lib = _ops(), _lib()
    N, H, W, Cin, Cout, R, stride, pad, dil = shape
    guard = 256 * Cout * 4
    if name == "strided-residual":
        case = ec.make_case(shape, dtype, dtype, 1, False, seed=5)
        full = torch.randint(-8, 9, (2, 9, 13, Cout), generator=torch.Generator().manual_seed(3)).to(dtype)

        def fn(put, writes):
            return {"y": ops.conv2d_nhwc(put(case.x), put(case.w), put(case.scale), put(case.bias), residual=put(full), relu=True,
                                         residual_stride=2)}
        got = _fenced(fn, dev, name, guard_bytes=guard)
        case.res = full[:, ::2, ::2].contiguous()
        ec.assert_bits_equal(got["y"], ec.reference(case)[0], "conv1x1 strided residual %s" % dtype, relu=1)
        return
    kw = {}
    M = N * ((H + 2 * pad - R) // stride + 1) * ((W + 2 * pad - R) // stride + 1)
    if name == "lib-splitk":
        assert lib.mega_conv2d_nhwc_workspace_bytes(M, Cout, R * R * Cin) > 0
        case = ec.conv_case(shape, dtype, dtype, 1, False)
    elif name == "conv64":
        assert _plan(shape, dtype, dtype)[0] == 6 and M % 256 != 0
        case = ec.conv_case(shape, dtype, dtype, 1, False)
    elif name.startswith("ksplit"):
        kw = {"ksplit": int(name[6:])}
        nb = lib.mega_conv2d_nhwc_ks_workspace_bytes(M, Cout, R * R * Cin, ops._DT[dtype], kw["ksplit"])
        assert nb > 0 and nb % (M * Cout * 4) == 0
        case = ec.conv_case(shape, dtype, dtype, 2, True)
    else:
        assert lib.mega_conv2d_nhwc_workspace_bytes(M, Cout, R * R * Cin) == 0
        case = ec.conv_case(shape, dtype, dtype, 1, True)
    got = _fenced(_conv_fn(case, **kw), dev, name, guard_bytes=guard)
    ec.assert_bits_equal(got["y"], ec.reference(case)[0], "conv %s %s %s" % (name, shape, dtype), relu=case.relu)


@pytest.mark.parametrize("ks", [1, 4])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_deconv_into_a_wider_buffer(dev, dtype, ks):
    """deconv4x4s2_into a placed [N, 9, 12, ldo] buffer of sentinels (ldo > Cs + C): the destination is registered with writes(),
    its slice equals the reference and the columns round the slice keep the sentinel"""
    ops = _ops()
    mult = 32 if dtype == F32 else 64
    N, H, W, Cin, C, Cs = sm.DECONV
    ldo = (Cs + C + 2 + mult - 1) // mult * mult
    H2, W2 = 2 * H + 1, 2 * W
    c = ec.deconv_case(sm.DECONV, dtype)
    xp = torch.zeros((N, H, W, (Cin + mult - 1) // mult * mult), dtype=dtype)
    xp[..., :Cin] = c.x
    w4 = ops.pack_deconv4x4s2(c.wt, dtype, mult)
    sentinel = torch.full((N, H2, W2, ldo), -7.0, dtype=dtype)

    def fn(put, writes):
        buf = writes(put(sentinel))
        ops.deconv4x4s2_into(put(xp), put(w4), put(c.bias.repeat(4)), buf, Cs, relu=2, ksplit=ks)
        return {"buf": buf}
    got = _fenced(fn, dev, "deconv into", guard_bytes=256 * ldo * 4, own=int(ks > 1))["buf"]      # (ksplit 1: no workspace)
    want, _ = ec.reference_deconv(c, 2, H2, W2)
    ec.assert_bits_equal(got[..., Cs:Cs + C].contiguous(), want, "deconv %s ksplit %d" % (dtype, ks), relu=2)
    assert bool((got[..., :Cs].float() == -7.0).all()) and bool((got[..., Cs + C:].float() == -7.0).all()), "written round the slice"


SP_TAIL = (1, 1, 37, 64, 72, 1, 1, 0, 1)       # M = 37, Cout = 72


@pytest.mark.parametrize("form", ["x3", "h2", "hi"])
def test_conv2d_sp_tails(dev, form):
    """conv2d_sp with planes output at M = 37, Cout = 72 in the x3, h2 and hi operand forms (the planes come from split_planes,
    fenced as well), the f32 output into a caller's out= buffer with ldo = Cout + 8, and linear_sp's split-K (x3) with the workspace of exactly mega_conv2d_nhwc_workspace_bytes"""
    ops = _ops()
    knobs = {"sexp": (-3, -2)} if form == "h2" else {}                     # (f16 planes: |y| < 65504, as ec.SP_TABLE's h2 rows)
    case = ec.make_sp_case(SP_TAIL, False, 1, False, seed=37 + len(form), form=form, **knobs)
    T = case.pdt
    w = {"x3": ops.split_conv_weight_x3, "h2": ops.split_conv_weight_h2}.get(form, lambda v: v.to(T))(case.w)

    def fn(put, writes):
        xp = ops.split_planes(put(case.x), T)
        y = ops.conv2d_sp(xp, put(w), put(case.scale), put(case.bias), relu=1, out_mode="planes", operands=form)
        return {"planes": xp, "y": y}
    got = _fenced(fn, dev, "conv2d_sp " + form, guard_bytes=256 * 2 * 72 * 4)
    ec.assert_bits_equal(got["planes"], torch.cat(ec.split_hi_lo(case.x, T), dim=-1), "split_planes")
    ec.assert_bits_equal(got["y"], ec.reference_sp(case, "planes")[0], "conv2d_sp %s planes" % form, relu=1)
    # f32 into the caller's [M, Cout + 8] buffer (ldo > Cout): a placed destination, nothing behind column Cout
    Mo, Co = SP_TAIL[2], SP_TAIL[4]

    def fn_out(put, writes):
        out = writes(put(torch.full((Mo, Co + 8), -7.0)))
        ops.conv2d_sp(ops.split_planes(put(case.x), T), put(w), put(case.scale), put(case.bias), relu=1, out_mode="f32",
                      operands=form, out=out)
        return {"out": out}
    got = _fenced(fn_out, dev, "conv2d_sp out= " + form, guard_bytes=256 * (Co + 8) * 4)["out"]
    assert bool((got[:, Co:] == -7.0).all()), "written behind column Cout"
    want = ec.reference_sp(case, "f32")[0]
    ec.assert_bits_equal(got[:, :Co].contiguous().view(want.shape), want, "conv2d_sp %s f32 out=" % form, relu=1)
    if form == "hi":
        return
    sk = ec.sp_splitk_case(form)
    M, K, Nout = ec.SP_SPLITK[form]
    Kk = ec.SP_FORMS[form][1] * K
    assert _lib().mega_conv2d_nhwc_workspace_bytes(M, Nout, Kk) == 3 * M * Nout * 4
    wk = {"x3": ops.split_conv_weight_x3, "h2": ops.split_conv_weight_h2}[form](sk.w).view(Nout, Kk)

    def fn_sk(put, writes):
        xp = ops.split_planes(put(sk.x.view(M, K)), sk.pdt)
        return {"y": ops.linear_sp(xp, put(wk), put(sk.bias), relu=True, operands=form)}
    got = _fenced(fn_sk, dev, "linear_sp split-K " + form, guard_bytes=256 * Nout * 4)
    want = ec.reference_sp(sk, "f32")[0]
    ec.assert_bits_equal(got["y"].view(want.shape), want, "linear_sp split-K %s" % form, relu=1)


def test_linear_transposed_tails(dev):
    """linear_transposed (16-bit, residual) and linear_transposed_x3 (through an X3Weight) at M = 37, ld = 64: the pad columns
    37 .. 63 are zero and nothing lands behind row Nout - 1"""
    ops = _ops()
    w, x, r = (t for t in _lt_inputs())
    M_, K_, N_, ld = sm.LT

    def fn(put, writes):
        return {"y": ops.linear_transposed(put(w.to(BF16)), put(x.to(BF16)), ld, residual=put(r.to(BF16)))}
    got = _fenced(fn, dev, "linear_transposed", guard_bytes=256 * ld * 4)["y"]
    ec.assert_bits_equal(got[:, :M_].contiguous(), ec.convert((w.double() @ x.double().t()) + r.double()[:, :M_], BF16), "linear_transposed")
    assert not bool(got[:, M_:].float().abs().any())
    M, K, Nout, ld3 = ec.SP_LINEAR_T
    case = ec.sp_linear_case(False)

    def fn3(put, writes):
        xw = ops.X3Weight(case.w.view(Nout, K), dev)                       # (packed on the host, moved whole: an input)
        return {"y": ops.linear_transposed(xw, put(case.x.view(M, K)), ld3)}
    got = _fenced(fn3, dev, "linear_transposed_x3", guard_bytes=256 * ld3 * 4)["y"]
    want = ec.reference_sp(case, "f32")[0]
    assert got.shape == (Nout, ld3) and bool((got[:, M:].contiguous().view(torch.int32) == 0).all()), "pad columns are not zero"
    ec.assert_bits_equal(got[:, :M].t().contiguous().view(want.shape), want, "linear_transposed_x3")


def _lt_inputs():
    M_, K_, N_, ld = sm.LT
    g = torch.Generator().manual_seed(5)
    return (torch.randint(-4, 5, (N_, K_), generator=g).float(), torch.randint(-8, 9, (M_, K_), generator=g).float(),
            torch.randint(-8, 9, (N_, ld), generator=g).float())


F8_KEYS = [k for k in fc.case_keys() if k[0] in (fc.SHAPES[0], fc.SHAPES[2])]


@pytest.mark.parametrize("key", F8_KEYS, ids=[fc.case_id(k) for k in F8_KEYS])
def test_conv_f8_tails(dev, key):
    """conv2d_nhwc_f8 on 5 x 7 (M = 35: fewer rows than any tile) in both tile classes (Cout 64: the 64-column tile, Cout 256:
    the 256-column one), every in x out combination: fp8 outputs are 1-byte elements, 35 x 64 of them"""
    ops = _ops()
    case = fc.conv_case(key)
    N, H, W, Cin, Cout, R = case.shape
    code = {"bf16": ops.BF16, "f8": ops.F8}
    assert _lib().mega_conv2d_nhwc_f8_plan(N, H, W, Cin, Cout, R, R, 1, case.pad, 1, code[case.in_kind], code[case.out_kind]) == \
        (256 if Cout % 256 == 0 else 64)

    def fn(put, writes):
        return {"y": ops.conv2d_nhwc_f8(put(case.x), put(case.wq), put(case.scale), put(case.bias),
                                        in_scale=case.in_scale if case.in_kind == "bf16" else None, out_scale=case.out_scale,
                                        pad=case.pad, relu=bool(case.relu))}
    got = _fenced(fn, dev, fc.case_id(key), guard_bytes=256 * Cout * 4)
    fc.assert_codes_equal(got["y"], fc.reference(case), fc.case_id(key))


# ===================================================================================================== fused blocks and stem
@pytest.mark.parametrize("ds", [False, True], ids=["bottleneck64", "bottleneck64_ds"])
def test_bottleneck_tails(dev, ds):
    """the fused layer1 blocks on 13 x 15: dense, and the even form whose compact output is 7 x 8"""
    ops = _ops()
    c = ec.make_bottleneck_case((1, 13, 15), BF16, seed=29 + int(ds), ds=ds)

    def fn(put, writes):
        args = [put(c.x)]
        for i in range(3):
            args += [put(c.w[i]), put(c.sb[i][0]), put(c.sb[i][1])]
        if ds:
            return {"y": ops.bottleneck64_ds(*args, put(c.w[3]), put(c.sb[3][0]), put(c.sb[3][1]))}
        return {"y": ops.bottleneck64(*args), "even": ops.bottleneck64(*args, subsample=True)}
    got = _fenced(fn, dev, "bottleneck64%s" % ("_ds" if ds else ""), guard_bytes=1 << 20)
    want, _ = ec.reference_bottleneck(c)
    ec.assert_bits_equal(got["y"], want, "bottleneck64%s 13 x 15" % ("_ds" if ds else ""), relu=1)
    if not ds:
        assert tuple(got["even"].shape[1:3]) == (7, 8)
        ec.assert_bits_equal(got["even"], want[:, ::2, ::2].contiguous(), "bottleneck64, even pixels", relu=1)


@pytest.mark.parametrize("hw", [(2, 31, 33), (1, 9, 7)])
def test_stem_tails(dev, hw):
    """stem (direct f32, direct bf16, matrix-core), stem_u8 and stem_pool (u8 and f32 input, bf16 and f16) on images of odd
    width whose pooled size (8 x 9, 3 x 2) is no multiple of the pooled tile"""
    ops = _ops()
    th, tw = ops.stem_pool_tile()
    N, H, W = hw
    Hp, Wp = ((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2
    assert W % 2 == 1 and Hp % th != 0 and Wp % tw != 0
    case = ec.stem_case(hw)
    wt = case.w.permute(1, 2, 3, 0).reshape(147, 64).contiguous()
    w160 = {dt: ops.pack_stem_weight_bf16(case.w, dt) for dt in (BF16, F16)}
    img = ec.stem_image(case, True)

    def fn(put, writes):
        u8, sc_, bi, im, wt_ = put(case.u8), put(case.scale), put(case.bias), put(img), put(wt)
        w16 = {dt: put(w160[dt]) for dt in (BF16, F16)}
        return {"f32": ops.stem(im, wt_, sc_, bi, F32), "bf16": ops.stem(im, wt_, sc_, bi, BF16),
                "mfma": ops.stem(im, wt_, sc_, bi, BF16, w_n160=w16[BF16]), "u8": ops.stem_u8(u8, w16[BF16], sc_, bi, case.mean, True),
                "pool_u8_bf16": ops.stem_pool(u8, w16[BF16], sc_, bi, case.mean, True),
                "pool_u8_f16": ops.stem_pool(u8, w16[F16], sc_, bi, case.mean, True),
                "pool_f32_bf16": ops.stem_pool(im, w16[BF16], sc_, bi), "pool_f32_f16": ops.stem_pool(im, w16[F16], sc_, bi)}
    got = _fenced(fn, dev, "stem %s" % (hw,))
    want16 = ec.reference_stem(case, BF16, True)[0]
    ec.assert_bits_equal(got["f32"], ec.reference_stem(case, F32, True)[0], "stem f32", relu=1)
    for k in ("bf16", "mfma", "u8"):
        ec.assert_bits_equal(got[k], want16, "stem " + k, relu=1)
    for dt in (BF16, F16):
        wantp = ec.reference_stem(case, dt, True, pool=True)[0]
        assert tuple(wantp.shape[1:3]) == (Hp, Wp)
        ec.assert_bits_equal(got["pool_u8_" + _NAME[dt]], wantp, "stem_pool u8", relu=1)
        ec.assert_bits_equal(got["pool_f32_" + _NAME[dt]], wantp, "stem_pool f32", relu=1)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pool_tails(dev, dtype):
    """maxpool3x3s2 and avgpool2x2_ceil on an odd x even map (7 x 10, C = 8) and an even x odd one"""
    ops = _ops()
    for shape in ((2, 7, 10, 8), (1, 10, 7, 8)):
        x = torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(sum(shape))).float()
        got = _fenced(lambda put, writes: {"max": ops.maxpool3x3s2(put(x.to(dtype))), "avg": ops.avgpool2x2_ceil(put(x.to(dtype)))},
                      dev, "pools %s" % (shape,))
        nchw = x.permute(0, 3, 1, 2)
        sc.assert_bits(got["max"], F.max_pool2d(nchw, 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(dtype), "max-pool")
        sc.assert_bits(got["avg"], F.avg_pool2d(nchw, 2, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous().to(dtype), "avg-pool")


# ===================================================================================================== spatial
ROI_C_MAX = 1032


@pytest.mark.parametrize("C", [8, ROI_C_MAX])
@pytest.mark.parametrize("K", [0, 1, 3])
def test_roi_align_tails(dev, K, C):
    """roi_align with K = 0, 1 and 3 ROIs, C = 8 and the lattice's 1032 channels, both output layouts, f32 and bf16; and
    roi_align_planes on the same ROIs"""
    ops = _ops()
    feat = sc.int_features(sc.MAP_B, sc.MAP_H, sc.MAP_W, ROI_C_MAX)[..., :C].contiguous()
    rois = sc.roi_lattice(7, sc.EXACT_GS)[:K].contiguous()
    ref = sc.oracle_roi_align(feat, rois, 7, 0) if K else torch.zeros((0, 49, C))

    def fn(put, writes):
        o = {}
        r = put(rois)
        for dt in (F32, BF16):
            f = put(feat.to(dt))
            o["nhwc-" + _NAME[dt]] = ops.roi_align(f, r, sc.SCALE, (7, 7), 0)
            o["nchw-" + _NAME[dt]] = ops.roi_align(f, r, sc.SCALE, (7, 7), 0, out_nhwc=False)
            if dt == F32:
                o["planes"] = ops.roi_align_planes(f, r, sc.SCALE, (7, 7), 0)
        return o
    got = _fenced(fn, dev, "roi_align K %d C %d" % (K, C))
    for dt in (F32, BF16):
        sc.assert_bits(got["nhwc-" + _NAME[dt]], ref.to(dt), "roi_align K %d C %d %s" % (K, C, dt))
        sc.assert_bits(got["nchw-" + _NAME[dt]].permute(0, 2, 3, 1).reshape(K, 49, C).contiguous(), ref.to(dt), "roi_align NCHW output")
    if K:
        sc.assert_bits(got["planes"], cpu_ops._planes(ref.reshape(K, -1), BF16).t, "roi_align_planes")
    else:
        assert got["planes"].shape[0] == 0


def test_flow_tails(dev):
    """dff_warp_scale on 5 x 9; flow_conv1_combine in its three addressing modes (contiguous, window order, group tables) on
    5 x 7; flow_pred_finish on 3 x 5 with ldz = 18; flow_level_assemble on the odd x even 9 x 12 target (after the deconv)"""
    ops = _ops()
    for dt in (F32, BF16):
        feats, flow, scale = (sc.int_features(1, 5, 9, 64, seed=5)[0].to(dt), sc.warp_lattice(5, 9)[0].contiguous(),
                              sc.pow2_scale(5, 9, 64, seed=5).to(dt))
        got = _fenced(lambda put, writes: {"y": ops.dff_warp_scale(put(feats), put(flow), put(scale))}, dev, "dff_warp_scale")
        sc.assert_bits(got["y"], cpu_ops.dff_warp_scale(feats, flow, scale), "dff_warp_scale %s" % dt)
        z, bias = mc.pred_inputs(2, 3, 5, 18)
        got = _fenced(lambda put, writes: {"y": ops.flow_pred_finish(put(z), put(bias), 2.5, dt)}, dev, "flow_pred_finish")
        ref, mag = mc.flow_pred_finish_f64(z, bias, 2.5)
        assert ((got["y"].double() - ref).abs() <= 10 * 2.0 ** -24 * mag + mc.half_ulp(ref, dt)).all()
    S, h, w = 6, 5, 7
    ab, bias = mc.conv1_inputs(S, h, w)
    orders = mc.orders_tensor(mc.conv1_group_orders(S, 2, S - 2))          # nwin > 0: [G, 1 + nwin] tables
    one = mc.orders_tensor([S - 1] + list(range(S)))                       # order (1-D): the key frame's slot is order[0], T = S
    modes = {"key": dict(key=2, T=S - 2), "order": dict(order=one), "group": dict(order=orders, nwin=S - 2)}

    def fn(put, writes):
        a, b = put(ab), put(bias)
        return {k: ops.flow_conv1_combine(a, b, BF16, **{n: (put(v) if isinstance(v, torch.Tensor) else v) for n, v in kw.items()})
                for k, kw in modes.items()}
    got = _fenced(fn, dev, "flow_conv1_combine")
    for k, kw in modes.items():
        assert torch.equal(got[k].view(torch.int16), cpu_ops.flow_conv1_combine(ab, bias, BF16, **kw).view(torch.int16)), k
    # one refinement level: Part A's flow-level case with its operands placed and the concatenation buffer a placed destination
    for dt in (F32, BF16):
        mult = 32 if dt == F32 else 64
        N, H, W, Cin, C, H2, W2, Cs = sm.LEVEL
        g = torch.Generator().manual_seed(N + Cin)
        x = torch.randint(-8, 9, (N, H, W, Cin), generator=g).to(dt)
        wt = torch.randint(-4, 5, (Cin, C, 4, 4), generator=g).float()
        b = torch.randint(-16, 17, (C,), generator=g).float()
        skip = torch.randint(-8, 9, (N, H2, W2, Cs), generator=g).to(dt)
        flow = torch.randint(-4, 5, (N, H, W, 2), generator=g).to(dt)
        wu = torch.randint(-2, 3, (2, 2, 4, 4), generator=g).float()
        bu = torch.randint(-4, 5, (2,), generator=g).float()
        ldo = (Cs + C + 2 + mult - 1) // mult * mult
        xp = torch.zeros((N, H, W, (Cin + mult - 1) // mult * mult), dtype=dt)
        xp[..., :Cin] = x
        w4 = ops.pack_deconv4x4s2(wt, dt, mult)

        def fn_level(put, writes):
            cc = writes(put(torch.full((N, H2, W2, ldo), -7.0, dtype=dt)))
            ops.deconv4x4s2_into(put(xp), put(w4), put(b.repeat(4)), cc, Cs, relu=2)
            return {"cc": ops.flow_level_assemble(put(skip), put(flow), put(wu), put(bu), cc, C)}
        got = _fenced(fn_level, dev, "flow level", guard_bytes=256 * ldo * 4, own=0)["cc"]       # (both write into cc only)
        dec, _ = ec.reference_deconv(SimpleNamespace(dtype=dt, x=x, wt=wt, bias=b), 2, H2, W2)
        up = F.conv_transpose2d(flow.double().permute(0, 3, 1, 2), wu.double(), bu.double(), stride=2)
        up = up[:, :, 1:1 + H2, 1:1 + W2].permute(0, 2, 3, 1).contiguous()
        want = torch.zeros((N, H2, W2, ldo), dtype=torch.float64)
        want[..., :Cs], want[..., Cs:Cs + C], want[..., Cs + C:Cs + C + 2] = skip.double(), dec.double(), up
        ec.assert_bits_equal(got, ec.convert(want, dt), "FlowNetS level concatenation %s" % dt)


FGFA_TAIL = (9, 5, 5, 7, 16, 8)         # S, T, H, W, Cf, Ce


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_fgfa_tails(dev, dtype):
    """fgfa_warp_aggregate with want_weights=True in its contiguous, window-order and _group forms, T = 5 frames of a 9-slot
    ring on 5 x 7 with 16 channels, and fgfa_pair_taps on 37 x 51, whose zero rows are part of the output"""
    ops = _ops()
    S, T, H, W, Cf, Ce = FGFA_TAIL
    ring, flow = mc.fgfa_ring(FGFA_TAIL, dtype)
    slots = mc.wrapped_slots(S, T)
    key_pos = T // 2
    idx = torch.tensor(slots)
    order = mc.orders_tensor(mc.order_row(slots, key_pos))
    rows = mc.group_slots(S, T, 2)
    orders = mc.orders_tensor([mc.order_row(r, key_pos) for r in rows])
    flows = mc.fgfa_flow(torch.Generator().manual_seed(2), 2 * T, H, W)

    def fn(put, writes):
        fl = put(flow[idx].contiguous())
        a, aw = ops.fgfa_warp_aggregate(put(ring[idx].contiguous()), fl, Cf, key_pos, want_weights=True)
        r = put(ring)
        b, bw = ops.fgfa_warp_aggregate(r, fl, Cf, 0, want_weights=True, order=put(order), flow_pos=key_pos)
        return {"out": a, "weights": aw, "ring": b, "ring_weights": bw,
                "group": ops.fgfa_warp_aggregate_group(r, put(flows), Cf, put(orders), key_pos)}
    got = _fenced(fn, dev, "fgfa_warp_aggregate %s" % dtype)
    ref, ref_w = mc.fgfa_aggregate_f64(ring, flow[idx], slots, key_pos, Cf)
    werr, err = (got["weights"].double() - ref_w).abs().max().item(), sm._relerr(got["out"], ref)
    assert werr < sm.FGFA_W_BOUND[dtype] and err < sm.FGFA_O_BOUND[dtype], (dtype, werr, err)
    assert torch.equal(got["ring"], got["out"]) and torch.equal(got["ring_weights"], got["weights"])
    assert torch.isfinite(got["group"].float()).all()
    if dtype == BF16:
        g = torch.Generator().manual_seed(91)
        refs, cur = torch.rand((3, 3, 37, 51), generator=g) * 255.0 - 110.0, torch.rand((1, 3, 37, 51), generator=g) * 255.0 - 110.0
        got = _fenced(lambda put, writes: {"taps": ops.fgfa_pair_taps(put(refs), put(cur), None, BF16)}, dev, "fgfa_pair_taps")["taps"]
        assert torch.equal(got.view(torch.int16), cpu_ops.fgfa_pair_taps(refs, cur, None, BF16).view(torch.int16))
        assert not bool(got[:, :3].float().abs().any()) and not bool(got[:, -3:].float().abs().any())


# ===================================================================================================== relation
POS_NK = (1, 63, 65, 97)


def test_position_logits_tails(dev):
    """position_logits in its precise, f32-row and tiled forms (Nq = 37, Nk = 70), and position_logits_batched with Nk = 1, 63,
    65 and 97 keys in the tiled layout: the pad keys' slots are inside the payload (never written, not compared), so for
    the batched form the bands are what is asserted, with the slots of the keys below Nk against float64"""
    ops = _ops()
    wg_t, bg, dm = sm._pos_weights()
    bq, bk = mc.pos_problem(37, 70)

    def fn(put, writes):
        q, k, w, b, d = put(bq), put(bk), put(wg_t), put(bg), put(dm)
        return {"rows": ops.position_logits(q, k, w, b, d, precise=True)[:, :, :70],
                "fast": ops.position_logits(q, k, w, b, d, precise=False)[:, :, :70],
                "tiled": sm._untile_pos(ops.position_logits(q, k, w, b, d, precise=False, tiled=BF16), 70)}
    got = _fenced(fn, dev, "position_logits")
    ref = mc.position_logits_f64(bq, bk, wg_t, bg).exp()
    for k in ("rows", "fast", "tiled"):
        err = (got[k].double().exp() - ref).abs()
        assert torch.isfinite(got[k]).all() and err.max() < 6e-3 and err.mean() < 1e-3, (k, err.max(), err.mean())
    probs = [mc.pos_problem(1 + 8 * i, nk) for i, nk in enumerate(POS_NK)]

    def fn_b(put, writes):
        outs = ops.position_logits_batched([put(a) for a, _ in probs], [put(b) for _, b in probs], put(wg_t), put(bg), put(dm),
                                           precise=False, tiled=BF16)
        return {"pos": [sm._untile_pos(o, nk) for o, nk in zip(outs, POS_NK)]}
    got = _fenced(fn_b, dev, "position_logits_batched")
    for (a, b), o in zip(probs, got["pos"]):
        err = (o.double().exp() - mc.position_logits_f64(a, b, wg_t, bg).exp()).abs()
        assert torch.isfinite(o).all() and err.max() < 6e-3, (tuple(o.shape), err.max())


ATTN_TAILS = [(1, 97), (33, 97), (1, 1500), (33, 1500), (33, 700, 800)]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32-stream"])
def test_attention_tails(dev, dtype):
    """relation_attention_batched with Nq = 1 and 33 query rows, one and three key-range splits (the workspace of exactly
    mega_relation_attention_workspace_bytes), two key segments inside wider buffers, and the f32 stream"""
    ops, lib = _ops(), _lib()
    assert sorted(set(lib.mega_relation_attention_splits(s[0], sum(s[1:]), 16) for s in ATTN_TAILS)) == [1, 3]
    assert lib.mega_relation_attention_workspace_bytes(33, 1500, 16) > 0 and lib.mega_relation_attention_workspace_bytes(33, 97, 16) == 0
    wg, bg, dm = mc.attn_pos_weights()
    its = [mc.attn_item(s, dtype, seed=70 + i) for i, s in enumerate(ATTN_TAILS)]

    def fn(put, writes):
        w, b, d = put(wg), put(bg), put(dm)
        items, defined = [], []
        for it in its:
            rq, rk = put(it["rq"]), put(it["rk"])
            if dtype == F32:
                pos = ops.position_logits(rq, rk, w, b, d, precise=True)
                defined.append(pos[:, :, :it["Nk"]])
            else:
                pos = ops.position_logits(rq, rk, w, b, d, precise=False, tiled=dtype)
                defined.append(sm._untile_pos(pos, it["Nk"]))
            dd = {"q": put(it["q"]), "Nk": it["Nk"], "resid": put(it["resid"]), "bias_v": put(it["bias_v"]), "pos": pos}
            if it["N2"]:
                N1, N2, a, c = it["N1"], it["N2"], it["a_cols"], it["b_cols"]
                big1, big2, kb1, kb2 = (put(it[n]) for n in ("big1", "big2", "kb1", "kb2"))
                dd.update(k=kb1[2:2 + N1], vt=big1[:, a:a + N1], N1=N1, k2=kb2[1:1 + N2], vt2=big2[:, c:c + N2])
            else:
                dd.update(k=put(it["k"]), vt=put(it["vt"]))
            items.append(dd)
        return {"pos": defined, "out": list(ops.relation_attention_batched(items))}
    got = _fenced(fn, dev, "relation_attention_batched %s" % dtype, slab_bytes=4 * SLAB_B)
    for i, it in enumerate(its):
        ref = mc.relation_attention_f64(it["q"], it["k"], it["vt"], it["Nk"], pos=got["pos"][i], resid=it["resid"], bias_v=it["bias_v"])
        o = got["out"][i]
        err = ((o.double() - ref).abs().max() / (ref.abs().max() + 1e-12)).item()
        assert torch.isfinite(o.float()).all() and err < mc.ATTN_BOUND[dtype], (ATTN_TAILS[i], dtype, err)


# ===================================================================================================== boxes
@pytest.mark.parametrize("n", [1, 64, 65, 2048, 2049])
def test_nms_tails(dev, n):
    """one box, one mask word, one box more, the last size of the mask form and the first of the lazy form; the workspace is
    what the wrapper asks of the library for that n"""
    boxes, scores, rank = bc.chain(n, 20)
    got = _fenced(lambda put, writes: {"keep": _ops().nms(_np(put, boxes), _np(put, scores), 0.5, strict_gt=True)}, dev, "nms %d" % n)
    bc.check_keep(got["keep"].numpy(), bc.chain_keep(rank, bc.CHAIN_PERIOD[(20, 0.5)]), "nms chain n %d vs closed form" % n)
    bc.check_keep(got["keep"].numpy(), native.nms(boxes, scores, 0.5, True), "nms chain n %d vs oracle" % n)


@pytest.mark.parametrize("form", sorted(sm.RPN_STALE))
def test_rpn_select_tails(dev, form):
    """the mask and the lazy form on two frames of which one stays below post_nms, rpn_out and the anchors placed"""
    frames = sm._rpn_frames(form)
    c = frames[0]
    rpn_out = torch.stack([k.rpn_out() for k in frames])

    def fn(put, writes):
        props, scores, cnt, index = _ops().rpn_select(put(rpn_out), put(c.cell), c.Hf, c.Wf, 16, c.pre, c.post, c.thr, c.min_size,
                                                      c.im_w, c.im_h, True, want_index=True)
        return {"props": props, "scores": scores, "count": cnt, "index": index}
    o = _fenced(fn, dev, "rpn_select " + form)
    assert any(int(o["count"][b]) < frames[b].post for b in range(2)), "no frame stays below post_nms"
    for b, k in enumerate(frames):
        bc.check_rpn((o["props"][b], o["scores"][b], int(o["count"][b]), o["index"][b]), k.oracle(), "%s frame %d" % (form, b))


@pytest.mark.parametrize("op", ["postprocess", "postprocess_batched", "postprocess_candidates_batched"])
def test_postprocess_tails(dev, op):
    """R = 70, a class without candidates, max_det between the two images' kept counts; logits, deltas and proposals placed"""
    ops = _ops()
    imgs = sm._post_images()
    c0 = imgs[0]
    cat = [torch.cat([getattr(c, n) for c in imgs]).contiguous() for n in ("logits", "deltas", "props")]
    nprop = torch.tensor([c.nprop for c in imgs], dtype=torch.int32)

    def fn(put, writes):
        if op == "postprocess":
            rows = {"count": [], "rows": []}
            for c in imgs:
                r = sm._post_rows(*ops.postprocess(put(c.logits), put(c.deltas), put(c.props), put(torch.tensor([c.nprop], dtype=torch.int32)),
                                                   *sm._post_args(c)))
                rows["count"] += r["count"]
                rows["rows"] += [tuple(t.clone() for t in r["rows"][0])]
            return rows
        lg, dl, pr = (put(t) for t in cat)
        if op == "postprocess_batched":
            return sm._post_rows(*ops.postprocess_batched(lg, dl, pr, 2, *sm._post_args(c0), nprop=put(nprop)))
        cb, cs = ops.postprocess_candidates_batched(lg, dl, pr, 2, c0.weights, c0.im_w, c0.im_h, c0.score_thresh, nprop=put(nprop))
        return {"scores": cs, "boxes": torch.where((cs >= 0)[..., None], cb, torch.zeros_like(cb))}
    o = _fenced(fn, dev, op)
    sm._POST()[op].check(o)


@pytest.mark.parametrize("op", sorted(sm.MERGE_KW))
def test_merge_tails(dev, op):
    """bbox_aug_merge and soft_merge (none / linear / gaussian / linear + vote) with the candidates placed"""
    frames, sizes, flips = sm._merge_frames("B")
    kw = sm.MERGE_KW[op]
    K = len(sizes)
    cb = torch.from_numpy(np.stack([np.stack([fr[k][0] for fr in frames]) for k in range(K)])).contiguous()
    cs = torch.from_numpy(np.stack([np.stack([fr[k][1] for fr in frames]) for k in range(K)])).contiguous()

    def fn(put, writes):
        if kw is None:
            return sm._post_rows(*_ops().bbox_aug_merge(put(cb), put(cs), sizes, flips, 0.001, 0.5, 30, True))
        return sm._post_rows(*_ops().soft_merge(put(cb), put(cs), sizes, flips, 0.001, 0.5, 30, True,
                                                **{sm._SOFT_KW[k]: v for k, v in kw.items()}))
    sm._MERGE()[op].check(_fenced(fn, dev, op))


# ===================================================================================================== copies and casts
def test_copy_tails(dev):
    """copy_blocks: 150-byte rows at 2-byte-aligned addresses, a block with a 1-byte tail (301-byte rows of u8), 63 segments
    (two launches), into placed destinations registered with writes(); multi_cat with 64 segments; cat_rows_cast_bf16"""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    vt = torch.randn((64, 300), generator=g).to(BF16)
    u8 = torch.randint(0, 256, (37, 301), generator=g, dtype=torch.uint8)
    big = torch.randn((300, 256), generator=g).to(BF16)
    pieces = [torch.randn((5, 64), generator=g), torch.randn((1, 64), generator=g)] + [torch.randn((2, 64), generator=g) for _ in range(60)]

    def fn(put, writes):
        v, u, b = put(vt), put(u8), put(big)
        d8 = writes(put(torch.full((37, 400), 7, dtype=torch.uint8)))
        d16 = writes(put(torch.full((64, 200), -7.0, dtype=BF16)))
        ops.copy_blocks([(d8[:, 3:304], u), (d16[:, 1:76], v[:, 75:150]), (d16[:, 77:80], v[:, 101:104])] +
                        [(d16[i:i + 1, 100:110], v[i:i + 1, 10:20]) for i in range(60)])
        many = [b[i * 3:i * 3 + 2] for i in range(60)]
        cols = [v[:, 0:75], v[:, 75:150], v[:, 151:154], v[:, 3:4]]
        outs = ops.multi_cat([(many, 0), (cols, 1)])
        return {"d8": d8, "d16": d16, "cat_rows": outs[0], "cat_cols": outs[1],
                "cat_cast": ops.cat_rows_cast_bf16([put(p) for p in pieces])}
    o = _fenced(fn, dev, "copy_blocks / multi_cat")
    w8 = torch.full((37, 400), 7, dtype=torch.uint8)
    w8[:, 3:304] = u8
    w16 = torch.full((64, 200), -7.0, dtype=BF16)
    w16[:, 1:76], w16[:, 77:80], w16[:60, 100:110] = vt[:, 75:150], vt[:, 101:104], vt[:60, 10:20]
    assert torch.equal(o["d8"], w8) and torch.equal(o["d16"].view(torch.int16), w16.view(torch.int16))
    assert torch.equal(o["cat_rows"], torch.cat([big[i * 3:i * 3 + 2] for i in range(60)], 0))
    assert torch.equal(o["cat_cols"], torch.cat([vt[:, 0:75], vt[:, 75:150], vt[:, 151:154], vt[:, 3:4]], 1))
    assert torch.equal(o["cat_cast"].view(torch.int16), torch.cat(pieces, 0).to(BF16).view(torch.int16))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2049])
def test_cast_tails(dev, n):
    """cast_half of n f32 elements to bf16 and f16 (below, at and above the 8-element vector; above one block), and
    split_planes / split_bf16x3 of one row of K = 8"""
    ops = _ops()
    g = torch.Generator().manual_seed(n)
    x = torch.randn((n,), generator=g) * 3
    row = torch.randn((1, 8), generator=g) * 100

    def fn(put, writes):
        r = put(row)
        return {"bf16": ops.cast_half(put(x), BF16), "f16": ops.cast_half(put(x), F16), "planes": ops.split_planes(r), "x3": ops.split_bf16x3(r)}
    o = _fenced(fn, dev, "casts n %d" % n)
    assert torch.equal(o["bf16"].view(torch.int16), x.to(BF16).view(torch.int16))
    assert torch.equal(o["f16"].view(torch.int16), x.to(F16).view(torch.int16))
    hi, lo = ec.split_hi_lo(row)
    assert torch.equal(o["planes"].view(torch.int16), torch.cat([hi, lo], -1).view(torch.int16))
    assert torch.equal(o["x3"].view(torch.int16), torch.cat([hi, lo, hi], -1).view(torch.int16))


# ===================================================================================================== frames
RESIZES = [("both-passes", (33, 50), (45, 67)), ("horizontal-only", (33, 50), (33, 67)), ("vertical-only", (33, 50), (45, 50)),
           ("same-size", (33, 50), (33, 50))]


@pytest.mark.parametrize("name,in_hw,out_hw", RESIZES, ids=[r[0] for r in RESIZES])
def test_resize_tails(dev, name, in_hw, out_hw):
    """resize_bilinear_u8 and _flip, N = 3 frames of 33 x 50 x 3 = 4950 bytes (no multiple of 4): both passes (tmp in use), one
    pass only, and the same size (copy / mirror)"""
    from mega.pytorch_amd import feed
    ops = _ops()
    frames = torch.randint(0, 256, (3,) + in_hw + (3,), generator=torch.Generator().manual_seed(33), dtype=torch.uint8)
    tables = feed.ResizeTables(in_hw, out_hw, dev)

    def fn(put, writes):
        f = put(frames)
        return {"resized": ops.resize_bilinear_u8(f, out_hw, tables), "flipped": ops.resize_bilinear_u8_flip(f, out_hw, tables),
                "mirror-without-tables": ops.resize_bilinear_u8_flip(f, in_hw, None) if in_hw == out_hw else None}
    o = _fenced(fn, dev, "resize " + name)
    want = cpu_ops.resize_bilinear_u8(frames, out_hw) if in_hw != out_hw else frames
    assert torch.equal(o["resized"], want) and torch.equal(o["flipped"], want.flip(2))
    if in_hw == out_hw:
        assert torch.equal(o["mirror-without-tables"], frames.flip(2))


def test_preprocess_frames_tails(dev):
    """preprocess_frames on N = 3 frames of 33 x 50, both channel orders"""
    from mega.pytorch_amd import synth
    frames = torch.randint(0, 256, (3, 33, 50, 3), generator=torch.Generator().manual_seed(50), dtype=torch.uint8)
    o = _fenced(lambda put, writes: {"bgr": _ops().preprocess_frames(put(frames), synth.PIXEL_MEAN, True),
                                     "rgb": _ops().preprocess_frames(put(frames), synth.PIXEL_MEAN, False)}, dev, "preprocess_frames")
    assert torch.equal(o["bgr"], synth.preprocess_cpu(frames))
    # (ToTensor's / 255, * 255, minus the mean: three separately rounded f32 operations, the channels in their own order)
    assert torch.equal(o["rgb"], frames.permute(0, 3, 1, 2).float() / 255.0 * 255.0 - torch.tensor(synth.PIXEL_MEAN).view(1, 3, 1, 1))


def _jpeg_host(info, bufs, extra=0):
    host = np.zeros((len(bufs), info.stride + extra), dtype=np.int16)
    for i, b in enumerate(bufs):
        host[i, :info.coef_elems] = b
    return torch.from_numpy(host)


JPEG_TAILS = ["1x1", "33x50-420-N3", "128x96-420", "128x96-422", "128x96-444", "128x96-gray", "out-slice"]


@pytest.mark.parametrize("name", JPEG_TAILS)
def test_jpeg_reconstruct_tails(dev, name):
    """jpeg_reconstruct at 1 x 1; 33 x 50 in 4:2:0 with N = 3 (frames of 4950 bytes: the byte-store path); 128 x 96 in all four
    samplings (the dword-store path); and into a caller's out= slice that starts off a dword"""
    from mega.pytorch_amd import jpeg
    ops = _ops()
    if name == "1x1":
        datas = [jpeg_cases.encode(jpeg_cases.picture(1, 1, 3), 2, 90)]
    elif name.startswith("128x96"):
        s = {"420": 2, "422": 1, "444": 0, "gray": None}[name.split("-")[1]]
        datas = [jpeg_cases.encode(jpeg_cases.picture(128, 96, 31, noise=(s == 0)), s, 92)] * 2
    else:
        datas = jpeg_cases.batch_case()
    info = jpeg.probe(datas[0])
    assert (info.width % 4 == 0) == name.startswith("128x96")
    coef = _jpeg_host(info, [ops.jpeg_entropy_decode(d, info) for d in datas])
    want = np.stack([jpeg_cases.pillow_rgb(d) for d in datas])
    if name != "out-slice":
        o = _fenced(lambda put, writes: {"rgb": ops.jpeg_reconstruct(put(coef), info)}, dev, "jpeg " + name)
        assert np.array_equal(o["rgb"].numpy(), want)
        return

    def fn(put, writes):
        big = writes(put(torch.full((3, info.height, info.width, 3), 7, dtype=torch.uint8)))
        assert big[1:].data_ptr() % 4 != 0
        ops.jpeg_reconstruct(put(coef)[1:], info, out=big[1:])
        return {"big": big}
    o = _fenced(fn, dev, "jpeg out= slice")
    assert np.array_equal(o["big"][1:].numpy(), want[1:]) and bool((o["big"][0] == 7).all())


def test_overlay_tails(dev):
    """overlay_detections at the smallest case of tests/test_demo_gpu.py (one 16 x 64 frame, 37 detections): it draws in place
    on the caller's frames, a placed destination"""
    from mega.pytorch_amd import demo
    atlas = demo.LabelAtlas(*demo.glyph_atlas(16))
    palette = demo.class_palette(len(demo.CATEGORIES))
    hw = rhw = (16, 64)
    frames = np.random.default_rng(5).integers(0, 256, (1,) + hw + (3,)).astype(np.uint8)
    box, score, label, counts = overlay_twin.random_detections(5, 1, 37, rhw)

    def fn(put, writes):
        f = writes(_np(put, frames))
        return {"frames": _ops().overlay_detections(f, _np(put, box), _np(put, score), _np(put, label), _np(put, counts), rhw, 0.0, 1,
                                                    _np(put, palette), atlas.to(dev))}
    o = _fenced(fn, dev, "overlay_detections", modules=_mods("ops"))
    want = overlay_twin.draw_batch(frames, box, score, label, counts, rhw, 0.0, 1, palette, atlas, demo.CATEGORIES)
    np.testing.assert_array_equal(o["frames"].numpy(), want)
    assert (want != frames).any()


# ===================================================================================================== evaluation and tracking
def _bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _seq_nms_hand(dev, name):
    from mega.pytorch_amd import seq_nms
    frames, videos, kw, keep, scores = seq_nms_cases.cases()[name]

    def fn(put, writes):
        out = seq_nms.seq_nms(seq_nms_twin.to_boxlists(frames), videos, device=dev, **kw)
        return {"n": [len(o) for o in out], "scores": [o.get_field("scores") for o in out]}
    o = _fenced(fn, dev, "seq_nms " + name, modules=_mods(*EVAL_MODULES), own=int(("seq_nms", name) not in NOTHING_LAUNCHED))
    assert o["n"] == [sum(k) for k in keep]
    for s, e in zip(o["scores"], scores):
        np.testing.assert_array_equal(_bits32(s.numpy()), _bits32(e))


def _tracks_hand(dev, name):
    from mega.pytorch_amd import tracks
    frames, videos, kw, ids, scores, table = tracks_cases.cases()[name]

    def fn(put, writes):
        out, tab = tracks.link(tracks_twin.to_boxlists(frames), videos, device=dev, **kw)
        return {"ids": [o.get_field("track_ids") for o in out], "scores": [o.get_field("scores") for o in out]}
    o = _fenced(fn, dev, "link_tracks " + name, modules=_mods(*EVAL_MODULES), own=int(("tracks", name) not in NOTHING_LAUNCHED))
    assert [t.tolist() for t in o["ids"]] == ids
    for s, e in zip(o["scores"], scores):
        np.testing.assert_array_equal(_bits32(s.numpy()), _bits32(e))


def _track_eval_hand(dev, name):
    from mega.pytorch_amd import track_eval
    case = track_eval_cases.cases()[name]
    keep = {}

    def fn(put, writes):
        preds, gt = track_eval_twin.to_inputs(case["preds"], case["gts"])
        r = track_eval.run(preds, gt, case["videos"], device=dev)
        keep["last"] = r
        return {k: r[k] for k in ("match", "matched_gt", "n_pos", "ap")}
    _fenced(fn, dev, "track_eval " + name, modules=_mods(*EVAL_MODULES))
    track_eval_cases.check(case, keep["last"])                              # (the run under the last polarity: the same bits)


def _motion_iou_set(dev, name):
    from mega.pytorch_amd import motion_iou
    c = motion_iou_cases.cases()[name]

    def fn(put, writes):
        v, cnt = motion_iou.run(c["gt"], c["videos"], c["window"], device=dev)
        return {"values": v, "counts": cnt}
    o = _fenced(fn, dev, "motion_iou " + name, modules=_mods(*EVAL_MODULES))
    tv, tc = motion_iou_twin.run(c["gt"].boxes, c["gt"].off, c["gt"].track_ids, c["videos"], c["window"])
    np.testing.assert_array_equal(o["counts"], tc)
    np.testing.assert_array_equal(o["values"].view(np.int64), tv.view(np.int64))


def _vid_eval_set(dev, name):
    from mega.pytorch_amd import vid_eval
    preds, gts, mot = vid_twin.make_frames(11, F=12, tie_scores=True, motion=True)

    def fn(put, writes):
        bl, gt = vid_twin.to_boxlists(preds, gts)
        r = vid_eval.match_and_ap(bl, gt, mot, device=dev)
        return {k: r[k] for k in ("match", "pred_ignore", "n_pos", "ap")}
    o = _fenced(fn, dev, "vid_eval", modules=_mods(*EVAL_MODULES))
    for ri, w in enumerate(vid_twin.evaluate(preds, gts, mot)):
        np.testing.assert_array_equal(o["match"][ri], w["match"])
        np.testing.assert_array_equal(o["n_pos"][ri], w["n_pos"])
        np.testing.assert_allclose(o["ap"][ri], w["ap"], rtol=0, atol=1e-9, equal_nan=True)


# hand-made sets without a box, a frame or a track: the entry point returns before it allocates or launches anything
NOTHING_LAUNCHED = {("seq_nms", "no_boxes"), ("tracks", "no_boxes"), ("tracks", "no_frames"), ("refine", "ids_all_minus_one")}


HAND_SETS = ([("seq_nms", n) for n in sorted(seq_nms_cases.cases())] + [("tracks", n) for n in sorted(tracks_cases.cases())] +
             [("track_eval", n) for n in sorted(track_eval_cases.cases())] +
             [("motion_iou", n) for n in sorted(motion_iou_cases.cases())] + [("vid_eval", "ties-motion")])
_HAND_RUN = {"seq_nms": _seq_nms_hand, "tracks": _tracks_hand, "track_eval": _track_eval_hand, "motion_iou": _motion_iou_set,
             "vid_eval": _vid_eval_set}


@pytest.mark.parametrize("family,name", HAND_SETS, ids=["%s-%s" % fn for fn in HAND_SETS])
def test_evaluation_hand_sets(dev, family, name):
    """The hand-made sets of seq_nms, link_tracks, tubelet_scores + tubelet_match (the table in LDS) and every motion_iou case
    (LDS, and the 130-box frame in the workspace), and vid_eval_match + vid_eval_ap on a tied set, through their modules'
    entry points with ops, seq_nms, tracks, track_eval, vid_eval, motion_iou, diagnose and flat fenced.  (The tubelet table in
    the workspace and proposal_recall_match: test_evaluation_table.)"""
    _HAND_RUN[family](dev, name)


def _packed_tracks(lengths, stride, seed):
    """tracks in one video, all starting in frame 0, track k with a box in every stride-th frame of its lengths[k] frames and
    in its last one (tests/test_track_refine_gpu.py's generator)"""
    rng = np.random.default_rng(seed)
    frames = []
    for t in range(max(lengths)):
        b, s, lab, ids = [], [], [], []
        for k in reversed(range(len(lengths))):
            if t < lengths[k] and (t % stride == 0 or t == lengths[k] - 1):
                x, y = 1000.0 * k + 0.5 * t + rng.normal(0, 1), 1000.0 * k + rng.normal(0, 1)
                b.append([x, y, x + 40, y + 30])
                s.append(rng.uniform(0.1, 1.0))
                lab.append(k + 1)
                ids.append(k)
        frames.append(track_refine_cases._frame(b, s, lab, ids))
    return frames


REFINE = sorted(track_refine_cases.cases()) + ["tile-boundary"]


@pytest.mark.parametrize("name", REFINE)
def test_refine_tracks(dev, name):
    """refine_tracks through tracks.refine on the hand-made cases and on two tracks of 256 slots each: the first ends exactly
    on the 256-slot tile boundary, where the second begins"""
    from mega.pytorch_amd import tracks
    if name == "tile-boundary":
        frames, videos, kw = _packed_tracks((256, 256), 3, seed=512), [(0, 256)], {"fill": True, "smooth": 1}
        want, info = track_refine_twin.refine(frames, videos, **kw)
        assert info["tracks"] == 2 and info["filled"] > 0
    else:
        frames, videos, kw, want, info = track_refine_cases.cases()[name]
    keep = {}

    def fn(put, writes):
        out, got_info = tracks.refine(track_refine_twin.to_boxlists(frames), videos, device=dev, **kw)
        keep["out"], keep["info"] = out, got_info
        return {"boxes": [o.bbox for o in out], "scores": [o.get_field("scores") for o in out]}
    _fenced(fn, dev, "refine_tracks " + name, modules=_mods(*EVAL_MODULES), own=int(("refine", name) not in NOTHING_LAUNCHED))
    assert_frames_equal(track_refine_twin.from_boxlists(keep["out"]), want)
    assert keep["info"] == info


DIAGNOSE = sorted(diagnose_cases.hand_cases()) + ["random"]


@pytest.mark.parametrize("name", DIAGNOSE)
def test_diagnose(dev, name):
    """diagnose_match through diagnose.evaluate_errors on the hand-made cases and the random base set: kinds, attributed boxes,
    per-GT detections and the IoU bits against the twin"""
    from mega.pytorch_amd import diagnose
    if name == "random":
        preds, gts = diagnose_cases.random_frames(diagnose_twin.frame_iou)[:2]
    else:
        preds, gts = diagnose_cases.hand_cases()[name]["preds"], diagnose_cases.hand_cases()[name]["gts"]

    def fn(put, writes):
        bl, gt = vid_twin.to_boxlists(preds, gts)
        r = diagnose.evaluate_errors(bl, gt, device=dev)
        return {k: r[k] for k in ("det_kind", "det_gt", "gt_det", "gt_state", "det_iou", "kind_counts", "confusion")}
    o = _fenced(fn, dev, "diagnose " + name, modules=_mods(*EVAL_MODULES))
    want = diagnose_twin.run(preds, gts)
    for k in ("det_kind", "det_gt", "gt_det", "gt_state", "kind_counts", "confusion"):
        np.testing.assert_array_equal(o[k], want[k], err_msg=k)
    np.testing.assert_array_equal(_bits32(o["det_iou"]), _bits32(want["det_iou"]))
