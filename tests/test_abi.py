"""CPU: the C-ABI library loads without a GPU and exports every symbol include/mega_hip.h declares
(no compute calls here), the ctypes signature table covers exactly that set, and the library reads no environment
variable that is not listed here."""
import glob
import os
import re

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
    assert sorted(_lib.SIGNATURES.keys()) == names


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
