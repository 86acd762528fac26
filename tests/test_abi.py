"""CPU: the C-ABI library loads without a GPU and exports every symbol include/mega_hip.h declares
(no compute calls here), the sources under csrc/ define exactly that set, the binding derived from the header (_lib.py's
parser) has the types and layouts the header states, and the library reads no environment variable that is not listed here."""
import ctypes
import glob
import os
import re

import pytest

from mega.pytorch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "mega_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mega_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    names = _declared()
    assert len(names) >= 14
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), "libmega_hip.so does not export " + n
    assert sorted(_lib.SIGNATURES.keys()) == names      # (this file's own scan of the header: the parser skipped none)
    assert sorted(_lib.PARAMS.keys()) == names and all(len(_lib.PARAMS[n]) == len(_lib.SIGNATURES[n][1]) for n in names)


def test_every_entry_point_is_declared_and_every_declaration_defined():
    """The sources include the header, so the compiler holds every definition to its prototype's types -- but an extern "C"
    definition WITHOUT a prototype still compiles and links, and a prototype without a definition fails only at load.  The
    set of names defined as `extern "C" ... mega_*(` under csrc/ must be the set the header declares."""
    csrc = os.path.join(ROOT, "mega", "pytorch_amd", "csrc")
    defined = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
        heads = re.findall(r'extern\s+"C"[^;{(]*?\b(mega_[a-z0-9_]+)\s*\([^;{}]*\)\s*([;{])', src)
        assert len(heads) == len(re.findall(r'extern\s+"C"', src)), os.path.basename(path) + ': an extern "C" this scan cannot read'
        for n, end in heads:
            assert end == "{", "%s: %s is declared again (the header is the one declaration)" % (os.path.basename(path), n)
            assert n not in defined, "%s is defined in %s and in %s" % (n, defined[n], os.path.basename(path))
            defined[n] = os.path.basename(path)
    declared = set(_declared())
    assert not set(defined) - declared, "defined under csrc/ but not declared in mega_hip.h: %s" % sorted(set(defined) - declared)
    assert not declared - set(defined), "declared in mega_hip.h but not defined under csrc/: %s" % sorted(declared - set(defined))
    # and the sources do see the header, with no second copy of what it defines
    common = open(os.path.join(csrc, "common.h")).read()
    assert re.search(r'#include\s+"[./]*include/mega_hip\.h"', common)
    for path in glob.glob(os.path.join(csrc, "*")):
        src = open(path).read() if path.endswith((".hip", ".h")) else ""
        assert not re.search(r"#define\s+MEGA_(F32|BF16|F16|OK|ERR_\w+)\b|Mega\w+DescC|MegaCopySegC", src), os.path.basename(path)


def test_parser_spot_checks_one_per_type_class():
    S, c = _lib.SIGNATURES, ctypes
    assert S["mega_cast_f32_to_half"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_size_t, c.c_int, c.c_void_p])
    assert S["mega_fgfa_pair_taps"] == (c.c_int, [c.c_void_p, c.c_longlong, c.c_void_p, c.c_longlong, c.c_void_p, c.c_void_p]
                                        + [c.c_int] * 4 + [c.c_void_p])
    assert S["mega_stem_pool_tile"] == (None, [c.c_void_p, c.c_void_p])
    assert S["mega_last_error_string"] == (c.c_char_p, [])
    assert S["mega_conv2d_nhwc"] == (c.c_int, [c.c_void_p] * 6 + [c.c_int] * 15 + [c.c_void_p])
    assert S["mega_flow_pred_finish"][1][:4] == [c.c_void_p, c.c_int, c.c_void_p, c.c_float]
    assert S["mega_nms_full_workspace_bytes"] == (c.c_size_t, [c.c_int])
    assert S["mega_copy_segments"] == (c.c_int, [c.c_void_p, c.c_int, c.c_void_p])      # a typed descriptor pointer
    assert _lib.PARAMS["mega_cast_f32_to_half"] == ("src", "dst", "n", "dtype", "stream")
    assert _lib.PARAMS["mega_last_error_string"] == () and _lib.PARAMS["mega_stem_pool_tile"] == ("rows", "cols")
    lib = _lib.load()
    for name, (res, args) in S.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_generated_structures_have_the_pinned_layout():
    """sizes and offsets as the static_asserts next to each struct's use pin them (relation.hip, assemble.hip)"""
    attn, pos, seg = (_lib.STRUCTS[n] for n in ("mega_attn_desc", "mega_pos_desc", "mega_copy_seg"))
    assert sorted(_lib.STRUCTS) == ["mega_attn_desc", "mega_copy_seg", "mega_pos_desc"]
    assert ctypes.sizeof(attn) == 144 and attn.k2.offset == 120 and attn.ws_bytes.offset == 72 and attn.ldq.offset == 80
    assert (attn.nk1.offset, attn.vt2.offset, attn.ldv2.offset, attn.reserved.offset) == (116, 128, 136, 140)
    assert [f[0] for f in attn._fields_] == ["q", "k", "vt", "pos", "pos_tiled", "resid", "bias_v", "out", "ws", "ws_bytes",
                                             "ldq", "ldk", "ldv", "ldp", "ldr", "ldo", "Nq", "Nk", "io_f32", "nk1", "k2", "vt2",
                                             "ldv2", "reserved"]
    assert ctypes.sizeof(pos) == 32 and [(f[0], getattr(pos, f[0]).offset) for f in pos._fields_] == [
        ("rois_q", 0), ("rois_k", 8), ("out", 16), ("Nq", 24), ("Nk", 28)]
    assert ctypes.sizeof(seg) == 40 and [(f[0], getattr(seg, f[0]).offset) for f in seg._fields_] == [
        ("src", 0), ("dst", 8), ("src_stride", 16), ("dst_stride", 24), ("rows", 32), ("row_bytes", 36)]
    assert seg.src_stride.size == 8 and seg.rows.size == 4
    for path, text in (("relation.hip", "sizeof(mega_attn_desc) == 144 && offsetof(mega_attn_desc, k2) == 120"),
                       ("relation.hip", "sizeof(mega_pos_desc) == 32"), ("assemble.hip", "sizeof(mega_copy_seg) == 40")):
        assert ("static_assert(" + text) in open(os.path.join(ROOT, "mega", "pytorch_amd", "csrc", path)).read()
    from mega.pytorch_amd import ops
    assert ops._AttnDesc is attn and ops._PosDesc is pos and ops._CopySeg is seg


@pytest.mark.parametrize("decl, what", [
    ("int mega_x(double v, int n);", "parameter `double v`"),                # a scalar type outside the set
    ("int mega_x(unsigned n, void* stream);", "parameter `unsigned n`"),
    ("int mega_x(int);", "parameter `int`"),                                 # unnamed
    ("double mega_x(int n);", "return type `double`"),
    ("float* mega_x(int n);", "return type `float*`"),
    ("typedef struct { int n[4]; } mega_s;", "field `int n[4]`"),
    ("typedef struct { double v; } mega_s;", "field `double v`"),
    ("struct mega_s { int n; };", "neither a prototype nor a typedef struct"),
    ("extern int mega_count;", "neither a prototype nor a typedef struct"),
])
def test_parser_refuses_what_is_outside_its_grammar(decl, what):
    ok = "/* a comment;\n   over two lines */\nint mega_ok(const float* a, long long n, size_t b, float f, void* stream);\n"
    sigs, params, structs = _lib.parse_header(ok)
    assert sigs == {"mega_ok": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_float,
                                               ctypes.c_void_p])} and params == {"mega_ok": ("a", "n", "b", "f", "stream")}
    with pytest.raises(ValueError) as e:
        _lib.parse_header(ok + "\n" + decl + "\n", "h.h")
    assert str(e.value).startswith("h.h:5: " + what), str(e.value)       # names the line
    with pytest.raises(ValueError, match="h.h:4: unterminated"):
        _lib.parse_header(ok + "int mega_x(int n)\n", "h.h")


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib.load()
    # NULL pointers / non-positive sizes must come back as MEGA_ERR_ARG before any launch
    assert lib.mega_conv2d_nhwc(None, None, None, None, None, None, 1, 1, 1, 64, 64, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1, None) == 1
    assert lib.mega_stem_conv_bn_relu(None, None, None, None, None, 1, 8, 8, 0, None) == 1
    assert lib.mega_nms_workspace_bytes(2, 6000) >= 2 * 6000 * 94 * 8
    assert lib.mega_nms(None, None, 9000, 0.5, 1, None, None, None, 0, None) == 1
    # round 6 (FlowNetS): NULL operands; a caller-chosen split count is clamped so that every K range holds a K-tile
    assert lib.mega_conv2d_nhwc_subpixel(None, None, None, None, 1, 4, 4, 64, 64, 2, 8, 8, 1, 128, 0, 1, 1, None, 0, None) == 1
    assert lib.mega_conv2d_nhwc_ks(None, None, None, None, None, None, 1, 1, 1, 64, 64, 1, 1, 1, 0, 1, 0, 0, 0, 1, 1, 2, None, 0, None) == 1
    assert lib.mega_flow_level_assemble(None, None, None, None, None, 1, 8, 8, 64, 64, 192, 4, 4, 1, 1, None) == 1
    assert lib.mega_flow_pred_finish(None, 64, None, 1.0, None, 1, 4, 4, 1, None) == 1
    assert lib.mega_flow_conv1_combine(None, None, None, 0, None, 1, 16, 0, 1, None) == 1
    assert lib.mega_fgfa_warp_aggregate_ring_pos(None, None, None, None, 3, 4, 4, 8, 8, None, 1, 1, None) == 1
    assert lib.mega_fgfa_warp_aggregate_ring_pos_batched(None, None, None, None, 3, 4, 4, 8, 8, None, 1, 2, 1, None) == 1
    assert lib.mega_conv2d_nhwc_ks_workspace_bytes(10, 8, 64 * 4, 1, 1) == 0           # one range: no workspace
    assert lib.mega_conv2d_nhwc_ks_workspace_bytes(10, 8, 64 * 4, 1, 3) == 2 * 10 * 8 * 4   # 4 K-tiles in 3 ranges of 2 -> 2 ranges
    assert lib.mega_conv2d_nhwc_ks_workspace_bytes(10, 8, 64 * 4, 1, 100) == 4 * 10 * 8 * 4   # never more ranges than K-tiles


# Every MEGA_* environment variable the HIP sources may read.  A kernel switch is a hidden global input: a variable left over
# in a shell silently changes which kernel runs, so a new one has to be added here on purpose.
ALLOWED_GETENV = {
    "MEGA_IGEMM_TILE",            # igemm.hip: forces the conv GEMM tile (tests/test_conv_dispatch.py and the conv tests set it)
}


def test_hip_sources_read_only_the_listed_environment_variables():
    csrc = os.path.join(ROOT, "mega", "pytorch_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert files
    found = {}
    for path in files:
        src = open(path).read()
        names = re.findall(r'getenv\s*\(\s*"([^"]*)"', src)
        # every getenv call must name its variable literally, or this scan would miss it
        assert len(names) == len(re.findall(r"\bgetenv\b", src)), os.path.basename(path) + ": getenv without a literal name"
        for n in names:
            found.setdefault(n, set()).add(os.path.basename(path))
    extra = {n: sorted(f) for n, f in found.items() if n not in ALLOWED_GETENV}
    assert not extra, "environment switches not in ALLOWED_GETENV: %r" % extra
