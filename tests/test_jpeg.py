"""CPU: the JPEG decode's definition (mega/pytorch_amd/jpeg.py) and its host half.  The numpy twin equals this machine's Pillow
byte for byte on every stream case -- a library difference shows HERE, not as a kernel failure -- the C probe and entropy
decoder (csrc/jpeg_entropy.h behind the C ABI) equal the twin's header fields, tables and coefficients exactly, whatever the
output buffer held; every refusal is raised; truncated and corrupted streams end in an error or a result, never a crash; faults
planted in the twin's stages are caught by the cases; and the decoder, compiled alone with the host compiler's address and
undefined-behaviour sanitizers, reads and writes nothing outside its buffers on the same streams."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases
import jpeg_twin
import poison
from mega.pytorch_amd import _lib, jpeg, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = jpeg_cases.stream_cases()
_TWIN = {}


def twin(name, data):
    """(header, coefficients, rgb) of a stream case, computed once"""
    if name not in _TWIN:
        h, buf = jpeg_twin.entropy_decode(data)
        rgb, fits = jpeg_twin.reconstruct(buf, h.width, h.height, h.sampling, want_fits=True)
        assert fits, name
        buf.setflags(write=False)
        rgb.setflags(write=False)
        _TWIN[name] = (h, buf, rgb)
    return _TWIN[name]


def test_the_cases_cover_what_they_claim():
    names = [n for n, _ in STREAMS]
    assert len(names) == len(set(names)) >= 114
    for w, h in jpeg_cases.SIZES:
        for s in ("444", "422", "420", "gray"):
            for q in ("q50", "q95", "q100", "optimised"):
                assert "%dx%d-%s-%s" % (w, h, s, q) in names
    assert sum("restart3" in n for n in names) == 4 and sum("noise-q100" in n for n in names) == 4
    for n, d in STREAMS:
        if "restart3" in n:
            assert jpeg.probe(d).restart > 0 and b"\xff\xd0" in d and b"\xff\xd1" in d
    # the noise cases do saturate the clamp
    assert any(twin(n, d)[2].min() == 0 and twin(n, d)[2].max() == 255 for n, d in STREAMS if "noise" in n)
    # the optimised cases carry other Huffman tables than the default ones
    d0, d1 = dict(STREAMS)["45x67-420-q95"], dict(STREAMS)["45x67-420-optimised"]
    assert jpeg_cases.segment(d0, 0xC4) != jpeg_cases.segment(d1, 0xC4)


@pytest.mark.parametrize("name, data", STREAMS, ids=[n for n, _ in STREAMS])
def test_twin_equals_pillow_and_c_decoder_equals_twin(name, data):
    h, buf, rgb = twin(name, data)
    want = jpeg_cases.pillow_rgb(data)
    assert rgb.shape == want.shape and np.array_equal(rgb, want), "the twin differs from this machine's Pillow"
    info = jpeg.probe(data)
    assert (info.width, info.height, info.ncomp, info.sampling) == (h.width, h.height, h.ncomp, h.sampling)
    assert info.blocks == tuple(h.blocks) and info.restart == h.restart and info.coef_elems == h.coef_elems == buf.size
    assert info.blocks == jpeg.geometry(h.width, h.height, h.sampling)
    assert np.array_equal(jpeg.make_info(h.width, h.height, h.sampling, h.restart).array, info.array)
    got = ops.jpeg_entropy_decode(data, info)
    assert got.dtype == np.int16 and np.array_equal(got, buf)
    # the staging buffer is re-used: what it held before must not show (poison.py's fills, 0x00 and 0xFF), nor a longer buffer
    for fill in sorted(poison._FILL.values()):
        out = np.full(info.stride + 24, fill * 0x0101, dtype=np.uint16).view(np.int16)
        assert ops.jpeg_entropy_decode(data, info, out) is out
        assert np.array_equal(out[:buf.size], buf)
        assert np.all(out[buf.size:].view(np.uint16) == fill * 0x0101), "wrote past its element count"


def test_batch_case_is_three_different_images_of_one_size():
    infos = [jpeg.probe(d) for d in jpeg_cases.batch_case()]
    assert all(i.same_frames(infos[0]) for i in infos) and infos[0].sampling == jpeg.S420
    rgbs = [jpeg_twin.decode(d) for d in jpeg_cases.batch_case()]
    assert not np.array_equal(rgbs[0], rgbs[1]) and not np.array_equal(rgbs[1], rgbs[2])
    for d, r in zip(jpeg_cases.batch_case(), rgbs):
        assert np.array_equal(r, jpeg_cases.pillow_rgb(d))


@pytest.mark.parametrize("name, data", jpeg_cases.refused_cases(), ids=[n for n, _ in jpeg_cases.refused_cases()])
def test_streams_outside_the_accepted_set_are_refused(name, data):
    with pytest.raises(jpeg.Unsupported):
        jpeg_twin.parse(data)
    with pytest.raises(jpeg.Unsupported):
        jpeg.probe(data)
    info = jpeg.make_info(17, 31, jpeg.S420)
    out = np.full(info.coef_elems, 0x5A5A, dtype=np.int16)
    with pytest.raises(jpeg.Unsupported):
        ops.jpeg_entropy_decode(data, info, out)


def test_another_size_or_sampling_than_expected_is_refused():
    d = jpeg_cases.encode(jpeg_cases.picture(17, 31, 1), 2)
    ops.jpeg_entropy_decode(d, jpeg.make_info(17, 31, jpeg.S420))
    for other in (jpeg.make_info(17, 31, jpeg.S444), jpeg.make_info(31, 17, jpeg.S420), jpeg.make_info(17, 31, jpeg.GRAY)):
        with pytest.raises(jpeg.Unsupported):
            ops.jpeg_entropy_decode(d, other)
    # a buffer below the frame's element count is a bad argument of the C entry point, with nothing written
    info = jpeg.probe(d)
    out = np.full(info.coef_elems, 0x5A5A, dtype=np.int16)
    a = np.frombuffer(d, dtype=np.uint8)
    assert _lib.load().mega_jpeg_entropy_decode(a.ctypes.data, a.size, info.array.ctypes.data, out.ctypes.data, out.size - 1) == 1
    assert np.all(out == 0x5A5A)
    assert _lib.load().mega_jpeg_probe(None, 10, info.array.ctypes.data) == 1
    assert _lib.load().mega_jpeg_probe(a.ctypes.data, 0, info.array.ctypes.data) == 1
    assert _lib.load().mega_jpeg_entropy_decode(a.ctypes.data, a.size, None, out.ctypes.data, out.size) == 1


@pytest.mark.parametrize("name, data", jpeg_cases.corrupt_cases(), ids=[n for n, _ in jpeg_cases.corrupt_cases()])
def test_each_broken_syntax_rule_ends_in_an_error(name, data):
    with pytest.raises(jpeg.Corrupt):
        jpeg_twin.entropy_decode(data)
    info = jpeg.probe(data) if name != "undefined-table" else None
    if info is None:
        with pytest.raises(jpeg.Unsupported):      # the probe cannot tell "corrupt" apart: the C ABI has one refusal code
            jpeg.probe(data)
        return
    with pytest.raises(jpeg.Corrupt):
        ops.jpeg_entropy_decode(data, info)


def _hostile_streams():
    good = jpeg_cases.encode(jpeg_cases.picture(45, 67, 11), 2, 90)
    rst = jpeg_cases.encode(jpeg_cases.picture(45, 67, 12), 1, 90, restart_marker_blocks=2)
    out = []
    for tag, d in (("420", good), ("422rst", rst)):
        out += [("%s-cut%d" % (tag, c), b, d) for c, b in jpeg_cases.truncations(d)]
        out += [("%s-flip%d" % (tag, i), b, d) for i, b in jpeg_cases.flips(d)]
    return out


def test_truncated_and_flipped_streams_error_or_decode():
    """an error or a result, never a crash or a hang; where the twin decodes, the C decoder gives the twin's coefficients"""
    outcomes = {"decoded": 0, "error": 0}
    for name, data, good in _hostile_streams():
        info = jpeg.probe(good)
        out = np.full(info.coef_elems + 16, 0x5A5A, dtype=np.int16)
        try:
            ops.jpeg_entropy_decode(data, info, out)
            got = True
        except (jpeg.Unsupported, jpeg.Corrupt):
            got = False
        try:
            want = jpeg_twin.entropy_decode(data)[1]
        except (jpeg.Unsupported, jpeg.Corrupt):
            want = None
        assert got == (want is not None), name
        if got:
            assert np.array_equal(out[:info.coef_elems], want), name
        assert np.all(out[info.coef_elems:] == 0x5A5A), name
        outcomes["decoded" if got else "error"] += 1
    assert outcomes["error"] >= 40 and outcomes["decoded"] >= 1, outcomes      # (a flip often leaves a decodable stream)


@pytest.mark.parametrize("fault, where", [("round78", "420"), ("edge", "420"), ("edge", "422"), ("transpose", "gray")])
def test_planted_faults_in_the_twin_are_caught(fault, where):
    caught = [n for n, d in STREAMS if where in n and not np.array_equal(jpeg_twin.decode(d, faults=(fault,)), twin(n, d)[2])]
    assert caught, "no %s case notices the planted fault %r" % (where, fault)
    # and by the coefficient-level cases, which the GPU test feeds to the kernels
    hit = 0
    for n, w, h, s, buf in jpeg_cases.coef_cases():
        hit += not np.array_equal(jpeg_twin.reconstruct(buf, w, h, s, faults=(fault,)), jpeg_twin.reconstruct(buf, w, h, s))
    assert hit or fault in ("round78", "edge"), fault      # (those cases have flat chroma within a block row: IDCT faults only)


def test_coefficient_cases_stay_inside_int16_after_dequantisation():
    kinds = set()
    for n, w, h, s, buf in jpeg_cases.coef_cases():
        rgb, fits = jpeg_twin.reconstruct(buf, w, h, s, want_fits=True)
        assert fits and rgb.shape == (h, w, 3), n
        assert buf.size == jpeg.make_info(w, h, s).coef_elems
        kinds.add(n.split("-")[0])
    assert kinds == {"dc", "each", "extremes", "checker", "dense"}
    each = dict((n, b) for n, w, h, s, b in jpeg_cases.coef_cases())["each-gray"][jpeg.QT_ELEMS:].reshape(-1, 64)
    assert sorted(int(np.flatnonzero(b)[0]) for b in each) == list(range(64)) and all(np.count_nonzero(b) == 1 for b in each)


def test_reconstruct_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert set(_lib.PARAMS) >= {"mega_jpeg_probe", "mega_jpeg_entropy_decode", "mega_jpeg_reconstruct",
                                "mega_jpeg_reconstruct_workspace_bytes"}
    assert _lib.SIGNATURES["mega_jpeg_probe"] == (_lib.c_int, [_lib.c_void_p, _lib.c_longlong, _lib.c_void_p])
    assert _lib.PARAMS["mega_jpeg_reconstruct"] == ("coef", "stride", "N", "H", "W", "sampling", "rgb", "ws", "ws_bytes", "stream")
    wsb = lib.mega_jpeg_reconstruct_workspace_bytes
    info = jpeg.make_info(45, 67, jpeg.S420)
    blocks = sum(bw * bh for bw, bh in info.blocks)
    assert wsb(1, 67, 45, jpeg.S420) == (64 * blocks + 255) // 256 * 256 and wsb(3, 67, 45, jpeg.S420) >= 3 * 64 * blocks
    # N, the sizes and the sampling code: the workspace twin answers 0 for what the launch refuses
    for bad in ((0, 67, 45, 3), (-1, 67, 45, 3), (65536, 67, 45, 3), (1, 0, 45, 3), (1, 67, 0, 3), (1, 65536, 45, 3),
                (1, 67, 65536, 3), (1, 67, 45, 4), (1, 67, 45, -1)):
        assert wsb(*bad) == 0, bad
    # with fake, never dereferenced, aligned addresses and a workspace of 0 bytes no call can reach a launch: a call that passes
    # the argument checks answers 3 (workspace too small), a refused one 1
    coef, rgb, ws = 0x10000, 0x20000, 0x30000
    rec = lib.mega_jpeg_reconstruct
    assert rec(coef, info.stride, 1, 67, 45, jpeg.S420, rgb, ws, 0, None) == 3
    for bad in ((0, 67, 45, 3), (65536, 67, 45, 3), (1, 0, 45, 3), (1, 67, 65536, 3), (1, 67, 45, 4), (1, 67, 45, -1)):
        assert rec(coef, 1 << 20, bad[0], bad[1], bad[2], bad[3], rgb, ws, 0, None) == 1, bad
    assert rec(coef, info.coef_elems - 8, 1, 67, 45, jpeg.S420, rgb, ws, 0, None) == 1       # stride below a frame
    assert rec(coef, info.stride + 4, 1, 67, 45, jpeg.S420, rgb, ws, 0, None) == 1           # stride not a multiple of 8
    assert rec(coef, -info.stride, 1, 67, 45, jpeg.S420, rgb, ws, 0, None) == 1
    assert rec(coef + 8, info.stride, 1, 67, 45, jpeg.S420, rgb, ws, 0, None) == 1           # coefficients off a 16-byte boundary
    # the output must start on a dword only where dwords are stored (W % 4 == 0); frames of 45 x 67 x 3 bytes are odd-sized,
    # so a slice of a batch of them starts anywhere
    i48 = jpeg.make_info(48, 67, jpeg.S420)
    assert rec(coef, i48.stride, 1, 67, 48, jpeg.S420, rgb + 2, ws, 0, None) == 1
    assert rec(coef, i48.stride, 1, 67, 48, jpeg.S420, rgb + 4, ws, 0, None) == 3
    assert rec(coef, info.stride, 1, 67, 45, jpeg.S420, rgb + 1, ws, 0, None) == 3
    assert rec(coef, info.stride, 1, 67, 45, jpeg.S420, rgb, ws + 4, 0, None) == 1
    for null in range(3):
        p = [coef, rgb, ws]
        p[null] = None
        assert rec(p[0], info.stride, 1, 67, 45, jpeg.S420, p[1], p[2], 0, None) == 1
    # the wrappers refuse host tensors: no CPU path
    import torch
    with pytest.raises(RuntimeError):
        ops.jpeg_reconstruct(torch.zeros((1, info.stride), dtype=torch.int16), info)


def test_docstring_states_the_definition():
    doc = jpeg.__doc__
    for k in (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172, 91881, 22554, 46802, 116130):
        assert str(k) in doc, k
    for phrase in ("fit int16", "clamps where the library's range table would wrap", "Unsupported", "CONST_BITS = 13",
                   "PASS1_BITS = 2", "never reads outside its input"):
        assert phrase in doc, phrase


def _host_compiler():
    for cc in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    return None


def test_entropy_decoder_alone_under_the_host_sanitizers(tmp_path):
    """tools/jpeg_entropy_check.cpp includes csrc/jpeg_entropy.h alone (no GPU library, nothing preloaded): built with
    -fsanitize=address,undefined, it must run over the truncated, flipped, refused and corrupt streams and exit 0"""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_entropy_check")
    base = [cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"), "-o", exe]
    # the runtimes linked into the program where the compiler can (the program then needs nothing from its environment)
    for extra in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode == 0:
            break
    if r.returncode != 0 and b"sanitize" in r.stdout.lower() and b"jpeg_entropy" not in r.stdout:
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stdout.decode()[-200:])
    assert r.returncode == 0, r.stdout.decode()
    files = []

    def put(name, data):
        p = tmp_path / name
        p.write_bytes(data)
        files.append(str(p))

    hostile = _hostile_streams()
    put("good", hostile[0][2])
    for name, data, _ in hostile:
        put(name, data)
    for name, data in jpeg_cases.refused_cases() + jpeg_cases.corrupt_cases() + STREAMS[::7]:
        put(name.replace(":", "_"), data)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    assert b"streams:" in r.stdout and b"0 decoded" not in r.stdout


def test_frame_source_decode_argument(tmp_path):
    from mega.pytorch_amd import feed
    frame = jpeg_cases.picture(45, 67, 1)
    (tmp_path / "000000.JPEG").write_bytes(jpeg_cases.encode(frame, 2))
    pattern = str(tmp_path / "%s.JPEG")
    with pytest.raises(ValueError, match="HIP device"):
        feed.FrameSource(pattern, "%06d", 1, "cpu", decode="device")
    with pytest.raises(ValueError, match="opener"):
        feed.FrameSource(pattern, "%06d", 1, "cuda", decode="device", opener=lambda f: frame)
    with pytest.raises(ValueError, match="decode must be"):
        feed.FrameSource(pattern, "%06d", 1, "cpu", decode="gpu")
    src = feed.FrameSource(pattern, "%06d", 1, "cpu", workers=1)      # the default stays the host decode
    assert src.decode_mode == "host" and src.host_fallbacks == 0 and src.in_hw == (67, 45)
    assert np.array_equal(src.fetch_original([0])[0].numpy(), jpeg_cases.pillow_rgb((tmp_path / "000000.JPEG").read_bytes()))
    src.close()
    # a reader stands in for img_dir / pattern
    src = feed.FrameSource(None, None, 1, "cpu", workers=1, reader=lambda f: (tmp_path / "000000.JPEG").read_bytes())
    assert src.in_hw == (67, 45)
    src.close()


def test_tools_take_the_decode_switch():
    import json
    import sys
    for tool in ("demo.py", "calibrate_f8.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "base", "--decode", "device", "--dry-run"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-1000:]
        assert json.loads(r.stdout.decode().strip())["decode"] == "device"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "demo.py"), "base", "--decode", "gpu", "--dry-run"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0
