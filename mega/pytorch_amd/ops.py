"""Tensor-level wrappers over the C ABI (include/mega_hip.h).

torch is used here only for device memory and the current HIP stream; every computation is a
hand-written gfx950 kernel in libmega_hip.so.  All wrappers raise if the library is missing, a
tensor is not on a HIP device, or a kernel call returns non-zero -- there is no CPU fallback.
"""
import contextlib
import ctypes
import threading
import math

import torch

from . import _lib
from . import f8

F32, BF16, F16 = 0, 1, 2
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_HALF = (torch.bfloat16, torch.float16)      # 16-bit matrix-core operand types


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("unsupported dtype %s (float32 / bfloat16 / float16 only)" % t.dtype)


_LAUNCH = threading.local()


def _stream():
    s = getattr(_LAUNCH, "s", None)
    return torch.cuda.current_stream().cuda_stream if s is None else s.cuda_stream


@contextlib.contextmanager
def launch_on(stream):
    """Inside the block this module's kernels are launched on `stream` (a torch.cuda.Stream; None = no change) while
    tensors are still ALLOCATED under torch's current stream: the way to run an op beside the current stream's work without
    handing the caching allocator blocks that belong to another stream (the caller orders the two streams with events
    and keeps the op's inputs alive until the streams have joined)."""
    prev = getattr(_LAUNCH, "s", None)
    _LAUNCH.s = stream if stream is not None else prev
    try:
        yield
    finally:
        _LAUNCH.s = prev


def profiling():
    return _PROF is not None


_NO_CPU = "mega.pytorch_amd ops need HIP device tensors (no CPU path)"


def _gpu(*ts):
    """the device check for tensors that reach a kernel inside a descriptor (_call checks its own arguments)"""
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(_NO_CPU)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(nbytes, device):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


class Profiler(object):
    """Per-kernel-family GPU time from HIP event pairs recorded on the launch stream (torch's current stream,
    the one every wrapper launches on), with the algorithmic FLOPs / bytes each launch stands for.  Used by
    bench.py for the roofline line; never enabled in the timed region."""

    def __init__(self):
        self.items = []

    def begin(self, family, flops=0.0, nbytes=0.0, detail=None):
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return [family, float(flops), float(nbytes), e0, detail]

    def end(self, tok):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        tok.append(e1)
        self.items.append(tok)

    def summary(self, by_detail=False):
        """{family: launches, ms, flops, bytes}; by_detail=True keys on (family, detail) -- detail = the GEMM shape
        "M x Cout x K (RxS)" of a conv / linear launch -- so that one layer can be told from another of the same tile."""
        torch.cuda.synchronize()
        out = {}
        for fam, fl, nb, e0, det, e1 in self.items:
            d = out.setdefault((fam, det) if by_detail else fam, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += nb
        return out


_PROF = None


def set_profiler(p):
    global _PROF
    _PROF = p


_ENTRY = {}      # entry point -> (its ctypes function, the positions of its pointer parameters, whether it ends in `stream`)


def _entry(name):
    fn = getattr(_lib.load(), name)
    takes_stream = _lib.PARAMS[name][-1:] == ("stream",)
    argtypes = _lib.SIGNATURES[name][1]
    ptrs = tuple(i for i, t in enumerate(argtypes[:len(argtypes) - takes_stream]) if t is ctypes.c_void_p)
    _ENTRY[name] = fn, ptrs, takes_stream
    return _ENTRY[name]


def _call(name, *args, prof=None, what=None):
    """One launch through the C ABI, as include/mega_hip.h declares `name`.  args: the prototype's parameters in order,
    without a trailing `stream` (the launch stream is appended).  Where the prototype takes a pointer, a tensor stands for
    its data_ptr() (a tensor that is not on a HIP device raises) and None for NULL; ctypes arrays and addresses pass as
    they are.  prof = (family, flops, bytes[, detail]): with a profiler set, its event pair brackets the C call itself.
    A non-zero return code raises through _lib.check under `what` (the entry point's name unless given)."""
    fn, ptrs, takes_stream = _ENTRY.get(name) or _entry(name)
    args = list(args)
    for i in ptrs:
        a = args[i]
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise RuntimeError(_NO_CPU)
            args[i] = a.data_ptr()
    if takes_stream:
        args.append(_stream())
    if prof is None or _PROF is None:
        rc = fn(*args)
    else:
        tok = _PROF.begin(*prof)
        rc = fn(*args)
        _PROF.end(tok)
    _lib.check(rc, what or name)


# ------------------------------------------------------------------------------------------------ conv / linear
def _igemm_family(M, Cout, K, dtype, shape=None):
    """name of the kernel instantiation a conv / linear is dispatched to (profiler families).  shape = (N, H, W, Cin, R,
    S, stride, pad, dil, ldo, has_residual, out dtype): the layer itself, asked through the launch path's own predicates;
    without it the (M, Cout, K) GEMM shape of a 1x1 layer / linear."""
    if shape is not None:
        N, H, W, Cin, R, S, stride, pad, dil, ldo, has_res, odt = shape
        t = _lib.load().mega_conv2d_nhwc_plan_ex(N, H, W, Cin, Cout, R, S, stride, pad, dil, ldo, int(has_res), _DT[dtype], _DT[odt])
    else:
        t = _lib.load().mega_conv2d_nhwc_plan(M, Cout, K, _DT[dtype])
    kind, t = t // 1000000, t % 1000000
    if kind == 6:
        return "conv64_bf16_3x3"
    # one family = one rocprofv3 symbol: igemm8_kernel<OT, ...> is instantiated per OUTPUT type, so a bf16 launch that writes
    # f32 (fc0's split-K partial sums, the RPN head's f32 logits) is a different symbol from the bf16-output launches of the
    # same tile ("_f32out")
    f32out = shape is not None and dtype in _HALF and (shape[-1] == torch.float32 or (kind in (7, 8) and _lib.load().mega_conv2d_nhwc_workspace_bytes(M, Cout, K) > 0))
    return "igemm%s_%s_%dx%d%s" % ({8: "8", 7: "8s"}.get(kind, ""), {torch.bfloat16: "bf16", torch.float16: "f16"}.get(dtype, "f32"),
                                   t // 1000, t % 1000, "_f32out" if f32out else "")


def conv2d_nhwc(x, w, scale=None, bias=None, residual=None, stride=1, pad=0, dil=1, relu=False, out_dtype=None,
                out=None, ksplit=None, residual_stride=1):
    """x [N,H,W,Cin] (contiguous), w [Cout,R,S,Cin] -> [N,Ho,Wo,Cout].  y = act(conv*scale + bias (+res));
    relu: False/0 none, True/1 ReLU, 2 LeakyReLU(0.1).  ksplit (int >= 1): the caller's split-K count
    (mega_conv2d_nhwc_ks: small-M / long-K layers of FlowNetS and the FGFA box head); None: the library's K-only rule.
    residual_stride s > 1 (a 1x1 / stride 1 conv on 16-bit tensors): residual is [N,Hr,Wr,Cout] with ceil(Hr / s) == Ho,
    ceil(Wr / s) == Wo and residual[:, ::s, ::s, :] is what is added, read in place (mega_conv2d_nhwc_rs)."""
    if residual_stride != 1:
        return _conv1x1_strided_residual(x, w, scale, bias, residual, int(residual_stride), relu, out_dtype, out, stride, pad, dil, ksplit)
    N, H, W, Cin = x.shape
    Cout, R, S, Cin2 = w.shape
    assert Cin == Cin2 and x.is_contiguous() and w.is_contiguous() and x.dtype == w.dtype
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    odt = x.dtype if out_dtype is None else out_dtype
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=odt, device=x.device)
    else:
        assert out.dtype == odt and out.shape == (N, Ho, Wo, Cout) and out.is_contiguous()
    if residual is not None:
        assert residual.shape == out.shape and residual.dtype == x.dtype and residual.is_contiguous()
    for v in (scale, bias):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout and v.is_contiguous())
    prof = None
    if _PROF is not None:      # family = the kernel symbol rocprofv3 would report for this launch
        prof = (_igemm_family(N * Ho * Wo, Cout, R * S * Cin, x.dtype,
                              (N, H, W, Cin, R, S, stride, pad, dil, Cout, residual is not None, odt)),
                2.0 * N * Ho * Wo * Cout * R * S * Cin,
                x.numel() * x.element_size() + w.numel() * w.element_size() + out.numel() * out.element_size()
                + (0 if residual is None else residual.numel() * residual.element_size()),
                "%dx%dx%d (%dx%d)" % (N * Ho * Wo, Cout, R * S * Cin, R, S))
    if x.numel() * x.element_size() >= 0x7FF00000 or w.numel() * w.element_size() >= 0x7FF00000:
        raise ValueError("conv2d_nhwc: operand of %.2f GiB; the kernels use 32-bit buffer offsets (< 2 GiB per operand): "
                         "lower the frame-stage batch (ClipEngine steps_per_batch) or split the call over M"
                         % (max(x.numel() * x.element_size(), w.numel() * w.element_size()) / 2.0 ** 30))
    if ksplit is not None:
        nb = _lib.load().mega_conv2d_nhwc_ks_workspace_bytes(N * Ho * Wo, Cout, R * S * Cin, _dt(x), int(ksplit))
        ws = _ws(nb, x.device) if nb else None
        _call("mega_conv2d_nhwc_ks", x, w, scale, bias, residual, out, N, H, W, Cin, Cout, R, S, stride, pad, dil, int(relu),
              Cout, Cout, _dt(x), _DT[odt], int(ksplit), ws, nb, prof=prof)
        return out
    nb = _lib.load().mega_conv2d_nhwc_workspace_bytes(N * Ho * Wo, Cout, R * S * Cin)     # > 0: long-K layer, split-K
    ws = _ws(nb, x.device) if nb else None
    _call("mega_conv2d_nhwc_ws", x, w, scale, bias, residual, out, N, H, W, Cin, Cout, R, S, stride, pad, dil, int(relu),
          Cout, Cout, _dt(x), _DT[odt], ws, nb, prof=prof, what="mega_conv2d_nhwc")
    return out


def _conv1x1_strided_residual(x, w, scale, bias, residual, rs, relu, out_dtype, out, stride, pad, dil, ksplit):
    N, H, W, Cin = x.shape
    Cout, R, S, Cin2 = w.shape
    assert rs > 1 and residual is not None and (R, S, stride, pad, dil) == (1, 1, 1, 0, 1) and ksplit is None
    assert Cin == Cin2 and x.is_contiguous() and w.is_contiguous() and x.dtype == w.dtype and x.dtype in _HALF
    assert out_dtype is None or out_dtype == x.dtype
    Hr, Wr = residual.shape[1:3]
    assert residual.dtype == x.dtype and residual.is_contiguous() and residual.shape[0] == N and residual.shape[3] == Cout
    assert -(-Hr // rs) == H and -(-Wr // rs) == W, "residual[:, ::s, ::s] must have the output's size"
    if out is None:
        out = torch.empty((N, H, W, Cout), dtype=x.dtype, device=x.device)
    else:
        assert out.dtype == x.dtype and out.shape == (N, H, W, Cout) and out.is_contiguous()
    for v in (scale, bias):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout and v.is_contiguous())
    if max(t.numel() * 2 for t in (x, w, out, residual)) >= 0x7FF00000:
        raise ValueError("conv2d_nhwc: operand of 2 GiB or more; the kernels use 32-bit buffer offsets")
    _call("mega_conv2d_nhwc_rs", x, w, scale, bias, residual, out, N, H, W, Cin, Cout, int(relu), Cout, Cout, Hr, Wr, rs,
          _dt(x), prof=("igemm8s_%s_rs" % {torch.bfloat16: "bf16", torch.float16: "f16"}[x.dtype], 2.0 * N * H * W * Cout * Cin,
                        (x.numel() + w.numel() + 2 * out.numel()) * 2.0,
                        "%dx%dx%d (1x1, residual stride %d)" % (N * H * W, Cout, Cin, rs)))
    return out


def pack_deconv4x4s2(wt, dtype, cin_mult):
    """nn.ConvTranspose2d(Cin, C, 4, stride=2).weight [Cin,C,4,4] -> the sub-pixel conv's operand [4 C, 2, 2, Cin padded to
    cin_mult]: w4[(a*2 + b)*C + co, r, s, ci] = wt[ci, co, a + 2 (1 - r), b + 2 (1 - s)]  (mega_conv2d_nhwc_subpixel)."""
    Cin, C = wt.shape[:2]
    cp = (Cin + cin_mult - 1) // cin_mult * cin_mult
    w4 = torch.zeros((2, 2, C, 2, 2, cp), dtype=torch.float32)
    wf = wt.detach().float().cpu()
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for s_ in range(2):
                    w4[a, b, :, r, s_, :Cin] = wf[:, :, a + 2 * (1 - r), b + 2 * (1 - s_)].t()
    return w4.view(4 * C, 2, 2, cp).to(dtype).contiguous()


def deconv4x4s2_into(x, w4, bias4, out, coff, relu=0, ksplit=1):
    """crop_like(act(ConvTranspose2d(Cin, C, 4, stride=2)(x))) written to out[..., coff:coff + C] (flownet.py:9-13,:40-52,:94-111):
    x [N,H,W,Cin] NHWC, w4 = pack_deconv4x4s2(weight), bias4 f32 [4 C] (the bias repeated four times) or None, out
    [N,H2,W2,ldo] contiguous (the level's concatenation buffer); crop_like's rule: the full map is (2H+2) x (2W+2); when its
    size differs from (H2, W2) one row / column is dropped at the top / left.  Only the slice is written: every other column
    of out keeps what it held (flow_level_assemble writes the rest of a level's buffer)."""
    N, H, W, Cin = x.shape
    C = w4.shape[0] // 4
    assert tuple(w4.shape) == (4 * C, 2, 2, Cin) and x.is_contiguous() and w4.is_contiguous() and out.is_contiguous()
    assert x.dtype == w4.dtype == out.dtype and out.shape[0] == N
    H2, W2, ldo = out.shape[1:]
    crop = 0 if (2 * H + 2, 2 * W + 2) == (H2, W2) else 1
    assert H2 + crop <= 2 * H + 2 and W2 + crop <= 2 * W + 2
    M = N * (H + 1) * (W + 1)
    nb = _lib.load().mega_conv2d_nhwc_ks_workspace_bytes(M, 4 * C, 4 * Cin, _dt(x), int(ksplit))
    ws = _ws(nb, x.device) if nb else None
    _call("mega_conv2d_nhwc_subpixel", x, w4, bias4, out, N, H, W, Cin, C, int(relu), H2, W2, crop, ldo, coff, _dt(x),
          int(ksplit), ws, nb,
          prof=("deconv_subpixel", 2.0 * M * 4 * C * 4 * Cin, (x.numel() + w4.numel() + N * H2 * W2 * C) * x.element_size(),
                "%dx%dx%d (2x2 sub-pixel)" % (M, 4 * C, 4 * Cin)))
    return out


def flow_conv1_combine(ab, bias, dtype, key=None, order=None, T=None, out=None, nwin=0):
    """FlowNetS flow_conv1 of the pairs (key frame, frame t) from the per-frame halves (mega_flow_conv1_combine): ab f32
    [S,h,w,128] = [A | B] of S frames, bias f32 [64] -> `dtype` [T,h,w,64] = leaky(A[key] + B[t] + bias), t = 0 .. T-1 (T = S by
    default).  The key frame's slot is `key` (host int) or order[0] (device i32: the engine's ring).
    nwin > 0: order i32 [G, 1 + nwin] = rows [key slot, slot of window position 0 .. nwin-1]: -> [G * nwin,h,w,64], pair
    g * nwin + t = (key frame of row g, the frame at window position t) -- exactly the pairs of G key frames, in window order."""
    S, h, w, c = ab.shape
    if nwin > 0:
        assert order is not None and order.dim() == 2 and order.shape[1] == nwin + 1
        T = order.shape[0] * nwin
    else:
        T = S if T is None else T
        assert T <= S
    assert c == 128 and ab.dtype == torch.float32 and ab.is_contiguous() and bias.dtype == torch.float32 and bias.numel() == 64
    assert dtype in _HALF and (key is not None or order is not None)
    assert order is None or (order.dtype == torch.int32 and order.is_contiguous())
    if out is None:
        out = torch.empty((T, h, w, 64), dtype=dtype, device=ab.device)
    assert out.dtype == dtype and tuple(out.shape) == (T, h, w, 64) and out.is_contiguous()
    _call("mega_flow_conv1_combine", ab, bias, order, -1 if key is None else int(key), out, T, h * w, int(nwin), _DT[dtype],
          prof=("flow_conv1_combine", 0.0, T * h * w * 64 * 6.0))
    return out


def flow_pred_finish(z, bias, scale, out_dtype):
    """second half of a FlowNetS flow prediction (mega_flow_pred_finish): z f32 [N,H,W,ldz] = the 1 x 1 conv of the level's map
    with the 18 (tap, channel) columns of Conv2d(Cin, 2, 3, padding=1) -> [N,H,W,2] = (sum of the shifted taps) * scale + bias."""
    N, H, W, ldz = z.shape
    assert z.dtype == torch.float32 and z.is_contiguous() and bias.dtype == torch.float32 and bias.numel() == 2
    out = torch.empty((N, H, W, 2), dtype=out_dtype, device=z.device)
    _call("mega_flow_pred_finish", z, ldz, bias, float(scale), out, N, H, W, _DT[out_dtype],
          prof=("flow_pred_finish", 0.0, N * H * W * (18 * 4.0 + 2 * out.element_size())))
    return out


def flow_level_assemble(skip, flow, w_up, b_up, out, C):
    """the rest of a FlowNetS refinement level's concatenation (mega_flow_level_assemble): out[..., :Cs] = skip,
    out[..., Cs+C:Cs+C+2] = crop_like(ConvTranspose2d(2, 2, 4, stride=2)(flow)) from the f32 weights w_up [2,2,4,4] / b_up [2],
    zeros up to out's channel stride; out[..., Cs:Cs+C] (the deconvolution's slice) is left alone."""
    N, H2, W2, Cs = skip.shape
    _, h, w, two = flow.shape
    assert two == 2 and out.shape[:3] == skip.shape[:3] and flow.shape[0] == N
    assert skip.is_contiguous() and flow.is_contiguous() and out.is_contiguous() and skip.dtype == flow.dtype == out.dtype
    assert w_up.dtype == torch.float32 and tuple(w_up.shape) == (2, 2, 4, 4) and w_up.is_contiguous() and b_up.dtype == torch.float32
    crop = 0 if (2 * h + 2, 2 * w + 2) == (H2, W2) else 1
    _call("mega_flow_level_assemble", skip, flow, w_up, b_up, out, N, H2, W2, Cs, C, out.shape[3], h, w, crop, _dt(skip),
          prof=("flow_level_assemble", 0.0, (skip.numel() + N * H2 * W2 * (out.shape[3] - C)) * skip.element_size()))
    return out


def bottleneck64(x, w1, s1, b1, w2, s2, b2, w3, s3, b3, subsample=False):
    """The fused identity bottleneck 256 -> 64 -> 64 (3x3) -> 256 (layer1 blocks 1, 2): x NHWC bf16 [N,H,W,256] ->
    relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + x) in one persistent kernel; same bits as the three conv2d_nhwc
    launches.  w1 [64,1,1,256], w2 [64,3,3,64], w3 [256,1,1,64] (OHWI bf16), s / b f32 FrozenBN scale / bias.
    subsample: the even pixels only -- y[:, ::2, ::2, :] as a contiguous [N,ceil(H/2),ceil(W/2),256] tensor, same bits (for a
    block whose only reader is a stride-2 1x1 conv: conv2 / conv3 / the residual / the stores run on a quarter of the pixels)."""
    N, H, W, C = x.shape
    assert C == 256 and x.dtype in _HALF and x.is_contiguous()
    assert tuple(w1.shape) == (64, 1, 1, 256) and tuple(w2.shape) == (64, 3, 3, 64) and tuple(w3.shape) == (256, 1, 1, 64)
    for t in (w1, w2, w3):
        assert t.dtype == x.dtype and t.is_contiguous()
    for v, n in ((s1, 64), (b1, 64), (s2, 64), (b2, 64), (s3, 256), (b3, 256)):
        assert v.dtype == torch.float32 and v.numel() == n and v.is_contiguous()
    if x.numel() * 2 >= 0x7FF00000:
        raise ValueError("bottleneck64: operand of %.2f GiB; 32-bit buffer offsets (< 2 GiB)" % (x.numel() * 2 / 2.0 ** 30))
    px = float(N * H * W)
    if subsample:
        out = torch.empty((N, (H + 1) // 2, (W + 1) // 2, 256), dtype=x.dtype, device=x.device)
        _call("mega_bottleneck64_even_fwd_dt", x, w1, s1, b1, w2, s2, b2, w3, s3, b3, out, N, H, W, _dt(x),
              prof=("bneck64_fused_even", 2.0 * px * (256 * 64 + (576 * 64 + 64 * 256) / 4.0), px * 512.0 + out.numel() * 2.0))
        return out
    out = torch.empty_like(x)
    _call("mega_bottleneck64_fwd_dt", x, w1, s1, b1, w2, s2, b2, w3, s3, b3, out, N, H, W, _dt(x),
          prof=("bneck64_fused", 2.0 * px * (256 * 64 + 576 * 64 + 64 * 256), px * 1024.0))
    return out


def bottleneck64_ds(x, w1, s1, b1, w2, s2, b2, w3, s3, b3, wd, sd, bd):
    """The fused FIRST block of layer1 (64 -> 64 -> 64 (3x3) -> 256 with the 1x1 downsample branch): x NHWC bf16 [N,H,W,64] ->
    relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1 x))))))) + bnd(convd(x))) [N,H,W,256]; same bits as the four conv2d_nhwc
    launches.  w1 [64,1,1,64], w2 [64,3,3,64], w3 / wd [256,1,1,64]."""
    N, H, W, C = x.shape
    assert C == 64 and x.dtype in _HALF and x.is_contiguous()
    assert tuple(w1.shape) == (64, 1, 1, 64) and tuple(w2.shape) == (64, 3, 3, 64)
    assert tuple(w3.shape) == (256, 1, 1, 64) and tuple(wd.shape) == (256, 1, 1, 64)
    for t in (w1, w2, w3, wd):
        assert t.dtype == x.dtype and t.is_contiguous()
    for v, n in ((s1, 64), (b1, 64), (s2, 64), (b2, 64), (s3, 256), (b3, 256), (sd, 256), (bd, 256)):
        assert v.dtype == torch.float32 and v.numel() == n and v.is_contiguous()
    out = torch.empty((N, H, W, 256), dtype=x.dtype, device=x.device)
    if out.numel() * 2 >= 0x7FF00000:
        raise ValueError("bottleneck64_ds: output of %.2f GiB; 32-bit buffer offsets (< 2 GiB)" % (out.numel() * 2 / 2.0 ** 30))
    px = float(N * H * W)
    _call("mega_bottleneck64_ds_fwd_dt", x, w1, s1, b1, w2, s2, b2, w3, s3, b3, wd, sd, bd, out, N, H, W, _dt(x),
          prof=("bneck64_fused", 2.0 * px * (64 * 64 + 576 * 64 + 2 * 64 * 256), px * 640.0))
    return out


def linear(x, w, bias=None, relu=False, residual=None, out_dtype=None, scale=None, ksplit=None):
    """x [M,K], w [Nout,K] (nn.Linear layout) -> [M,Nout].  ksplit: the caller's split-K count (conv2d_nhwc)."""
    if isinstance(w, X3Weight):      # split-precision: f32 in, f32 out
        assert x.dtype == torch.float32 and residual is None and scale is None and out_dtype in (None, torch.float32)
        return linear_sp(split_planes(x.contiguous()), w.w3, bias, relu=relu)
    M, K = x.shape
    y = conv2d_nhwc(x.view(M, 1, 1, K), w.view(w.shape[0], 1, 1, K), scale=scale, bias=bias,
                    residual=None if residual is None else residual.view(M, 1, 1, -1), relu=relu,
                    out_dtype=out_dtype, ksplit=ksplit)
    return y.view(M, w.shape[0])


def stem(x_nchw, w_tap64, scale, bias, out_dtype, w_n160=None):
    """x [N,3,H,W] f32 -> conv7x7 s2 + BN + ReLU -> NHWC [N,Ho,Wo,64].  f32: direct conv with w_tap64 [147,64] f32;
    bf16: matrix-core kernel with w_n160 = bf16 [64,176] (see pack_stem_weight_bf16)."""
    N, C, H, W = x_nchw.shape
    assert C == 3 and x_nchw.dtype == torch.float32 and x_nchw.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, Ho, Wo, 64), dtype=out_dtype, device=x_nchw.device)
    prof = ("stem", 2.0 * N * Ho * Wo * 64 * 147, x_nchw.numel() * 4 + out.numel() * out.element_size())
    if out_dtype == torch.bfloat16 and w_n160 is not None:
        assert w_n160.dtype == torch.bfloat16 and tuple(w_n160.shape) == (64, 176) and w_n160.is_contiguous()
        _call("mega_stem_conv_bn_relu_bf16", x_nchw, w_n160, scale, bias, out, N, H, W, prof=prof, what="mega_stem_conv_bn_relu")
    else:
        _call("mega_stem_conv_bn_relu", x_nchw, w_tap64, scale, bias, out, N, H, W, _DT[out_dtype], prof=prof)
    return out


def stem_u8(frames_u8, w_n160, scale, bias, mean, to_bgr=True):
    """uint8 frames [N,H,W,3] RGB -> preprocess (BGR*255 - mean) + conv7x7 s2 + BN + ReLU -> NHWC bf16 [N,Ho,Wo,64] in ONE
    kernel (the bf16 matrix-core stem with the preprocessing on its patch load): same bits as
    stem(preprocess_frames(frames_u8), ...)."""
    N, H, W, C = frames_u8.shape
    assert C == 3 and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
    assert w_n160.dtype == torch.bfloat16 and tuple(w_n160.shape) == (64, 176) and w_n160.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, Ho, Wo, 64), dtype=torch.bfloat16, device=frames_u8.device)
    _call("mega_stem_conv_bn_relu_bf16_u8", frames_u8, w_n160, scale, bias, out, N, H, W, float(mean[0]), float(mean[1]),
          float(mean[2]), int(to_bgr), prof=("stem", 2.0 * N * Ho * Wo * 64 * 147, frames_u8.numel() + out.numel() * 2))
    return out


def stem_pool(x, w_n160, scale, bias, mean=None, to_bgr=True):
    """resnet.py:355-366 in ONE kernel (bf16): conv7x7 s2 + BN + ReLU + max_pool2d(3, 2, 1) -> NHWC bf16 [N,Hp,Wp,64].  x =
    uint8 frames [N,H,W,3] RGB (preprocessing on the patch load, `mean` required) or the preprocessed f32 NCHW image.  Same
    bits as maxpool3x3s2(stem[_u8](...)); the stem's own map never reaches HBM."""
    u8 = x.dtype == torch.uint8
    if u8:
        N, H, W, C = x.shape
        assert mean is not None
    else:
        N, C, H, W = x.shape
        assert x.dtype == torch.float32
        mean = (0.0, 0.0, 0.0)
    assert C == 3 and x.is_contiguous()
    assert w_n160.dtype in _HALF and tuple(w_n160.shape) == (64, 176) and w_n160.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    out = torch.empty((N, Hp, Wp, 64), dtype=w_n160.dtype, device=x.device)      # (the weights' 16-bit type is the output's)
    _call("mega_stem_pool_dt", x, int(u8), w_n160, scale, bias, out, N, H, W, float(mean[0]), float(mean[1]),
          float(mean[2]), int(to_bgr), _dt(w_n160),
          prof=("stem", 2.0 * N * Ho * Wo * 64 * 147, x.numel() * x.element_size() + out.numel() * 2))
    return out


def stem_pool_tile():
    """(rows, columns) of the pooled tile that is one unit of stem_pool's work, as the kernel was compiled."""
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    _lib.load().mega_stem_pool_tile(ctypes.byref(th), ctypes.byref(tw))
    return th.value, tw.value


def pack_stem_weight_bf16(w_oihw, dtype=torch.bfloat16):
    """conv1.weight [64,3,7,7] -> bf16 (or f16) [64,176]: column k = ((c*7+r)*8 + s for the 7 taps s of kernel row (c, r); the
    8th column of every group and columns 168..175 are zero (the kernel reads 8 consecutive patch pixels per group)."""
    w = torch.zeros((64, 22, 8), dtype=torch.float32, device=w_oihw.device)
    w[:, :21, :7] = w_oihw.detach().float().reshape(64, 21, 7)
    w = w.reshape(64, 176)
    return w.to(dtype).contiguous()


def maxpool3x3s2(x):
    N, H, W, C = x.shape
    assert x.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    _call("mega_maxpool3x3s2_nhwc", x, out, N, H, W, C, _dt(x),
          prof=("maxpool", 0.0, (x.numel() + out.numel()) * x.element_size()))
    return out


# ------------------------------------------------------------------------------------------------ ROIAlign
def roi_align(feat, rois, spatial_scale, pooled, sampling_ratio, in_nhwc=True, out_nhwc=True):
    """feat NHWC [B,H,W,C] (or NCHW when in_nhwc=False); rois [K,5] f32 -> [K,ph*pw,C] (or [K,C,ph,pw])."""
    if in_nhwc:
        B, H, W, C = feat.shape
    else:
        B, C, H, W = feat.shape
    ph, pw = pooled
    K = rois.shape[0]
    assert feat.is_contiguous() and rois.dtype == torch.float32 and rois.is_contiguous() and rois.shape[1] == 5
    shape = (K, ph * pw, C) if out_nhwc else (K, C, ph, pw)
    out = torch.empty(shape, dtype=feat.dtype, device=feat.device)
    _call("mega_roi_align_fwd", feat, rois, out, K, C, H, W, float(spatial_scale), ph, pw, int(sampling_ratio),
          int(in_nhwc), int(out_nhwc), _dt(feat), _dt(feat),
          prof=("roi_align", 0.0, out.numel() * out.element_size() + feat.numel() * feat.element_size()))
    return out


def roi_align_planes(feat, rois, spatial_scale, pooled, sampling_ratio, dtype=torch.bfloat16):
    """roi_align on f32 NHWC features, the pooled rows as split-precision planes: -> Planes [K, ph*pw*C] (t = bf16 / f16
    [K, 2*ph*pw*C]), without the f32 tensor in between.  Large launches (C / 4 a multiple of 8 channel vectors, adaptive grid) run
    the separable per-ROI form of the 16-bit kernels: split_planes(roi_align(...)) to f32 round-off; small ones the
    exact-term-order kernel: bit for bit."""
    B, H, W, C = feat.shape
    ph, pw = pooled
    K = rois.shape[0]
    assert feat.dtype == torch.float32 and feat.is_contiguous() and rois.dtype == torch.float32 and rois.is_contiguous()
    assert rois.shape[1] == 5 and C % 4 == 0
    out = torch.empty((K, 2 * ph * pw * C), dtype=dtype, device=feat.device)
    _call("mega_roi_align_fwd_planes_dt", feat, rois, out, K, C, H, W, float(spatial_scale), ph, pw, int(sampling_ratio),
          _DT[dtype], prof=("roi_align", 0.0, out.numel() * 2 + feat.numel() * 4))
    return Planes(out, ph * pw * C)


# ------------------------------------------------------------------------------------------------ NMS
def nms(dets, scores, thr, strict_gt=True):
    """Kept ORIGINAL indices ascending (int64), reference mega_core._C.nms semantics.  One host sync (size)."""
    n = dets.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=dets.device)
    if n > 8192:
        raise ValueError("nms: %d boxes; the single-block sort / scan kernels take at most 8192 per problem" % n)
    dets = dets.contiguous().float()
    scores = scores.contiguous().float()
    keep = torch.empty((n,), dtype=torch.int64, device=dets.device)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dets.device)
    nb = _lib.load().mega_nms_full_workspace_bytes(n)
    ws = _ws(nb, dets.device)
    _call("mega_nms", dets, scores, n, float(thr), int(strict_gt), keep, cnt, ws, nb)
    return keep[: int(cnt.item())]


def rpn_select(rpn_out, cell_anchors, Hf, Wf, anchor_stride, pre_nms, post_nms, nms_thresh, min_size, im_w, im_h,
               strict_gt=True, want_index=False, hold=None):
    """rpn_out [B,Hf*Wf,5A] f32 -> proposals [B,post_nms,4], scores [B,post_nms], counts [B] (all on device).
    The rows past counts[b] are written too: zero proposals, zero scores.
    want_index: also the kept proposals' flat anchor indices (y*Wf + x)*A + a, [B,post_nms] i32, -1 past the count.
    hold (a list): the workspace is appended to it -- a caller that launches this on a side stream (launch_on) keeps it
    alive until the streams have joined, so that the allocator cannot hand the block to the current stream's next op."""
    B = rpn_out.shape[0]
    A = cell_anchors.shape[0]
    ldc = rpn_out.shape[-1]
    assert rpn_out.dtype == torch.float32 and rpn_out.is_contiguous() and rpn_out.numel() == B * Hf * Wf * ldc
    k = min(pre_nms, Hf * Wf * A)
    if k > 8192:
        raise ValueError("rpn_select: PRE_NMS_TOP_N = %d; the on-chip sort takes at most 8192 candidates per frame "
                         "(MODEL.RPN.PRE_NMS_TOP_N_TEST / MODEL.VID.RPN.REF_PRE_NMS_TOP_N)" % k)
    props = torch.empty((B, post_nms, 4), dtype=torch.float32, device=rpn_out.device)
    scores = torch.empty((B, post_nms), dtype=torch.float32, device=rpn_out.device)
    cnt = torch.empty((B,), dtype=torch.int32, device=rpn_out.device)
    nb = _lib.load().mega_rpn_select_workspace_bytes(B, k)
    ws = _ws(nb, rpn_out.device)
    index = torch.empty((B, post_nms), dtype=torch.int32, device=rpn_out.device) if want_index else None
    _call("mega_rpn_select_idx", rpn_out, cell_anchors, B, Hf, Wf, A, ldc, anchor_stride, pre_nms, post_nms, float(nms_thresh),
          int(strict_gt), float(min_size), float(im_w), float(im_h), props, scores, cnt, index, ws, nb,
          prof=("rpn_select", 0.0, rpn_out.numel() * 4))
    if hold is not None:
        hold.append(ws)
    return (props, scores, cnt, index) if want_index else (props, scores, cnt)


def postprocess(logits, deltas, props, nprop, weights, im_w, im_h, score_thresh, nms_thresh, max_det,
                strict_gt=True, want_probs=False):
    """One image: returns (boxes [cap,4], scores [cap], labels [cap] i64, count [1] i32 device[, probs]), cap = (NC-1) * R.
    The detections are the first `count` rows; the rows from `count` on are not written (torch.empty: whatever the
    allocator's block held) and no part of the result."""
    R, NC = logits.shape
    if R > 1024:
        raise ValueError("postprocess: %d proposals; the per-class sort takes at most 1024 per image "
                         "(MODEL.RPN.POST_NMS_TOP_N_TEST)" % R)
    cap = (NC - 1) * R
    dev = logits.device
    ob = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((cap,), dtype=torch.float32, device=dev)
    ol = torch.empty((cap,), dtype=torch.int64, device=dev)
    oc = torch.zeros((1,), dtype=torch.int32, device=dev)
    probs = torch.empty((R, NC), dtype=torch.float32, device=dev) if want_probs else None
    nb = _lib.load().mega_postprocess_workspace_bytes(R, NC)
    ws = _ws(nb, dev)
    assert logits.dtype == torch.float32 and deltas.dtype == torch.float32 and props.dtype == torch.float32
    assert logits.is_contiguous() and deltas.is_contiguous() and props.is_contiguous()
    wx, wy, ww, wh = weights
    _call("mega_postprocess", logits, deltas, props, nprop, R, NC, wx, wy, ww, wh, float(im_w), float(im_h),
          float(score_thresh), float(nms_thresh), int(strict_gt), int(max_det), ob, os_, ol, oc, probs, ws, nb,
          prof=("postprocess", 0.0, (logits.numel() + deltas.numel()) * 4))
    return (ob, os_, ol, oc, probs) if want_probs else (ob, os_, ol, oc)


def postprocess_batched(logits, deltas, props, B, weights, im_w, im_h, score_thresh, nms_thresh, max_det,
                        strict_gt=True, nprop=None):
    """B images of R = rows / B proposals each (logits [B*R,NC], deltas [B*R,NC*4], props [B*R,4]) in one launch chain.
    Returns (boxes [B,cap,4], scores [B,cap], labels [B,cap] i64, counts [B] i32 device); image b has the bits of
    postprocess() on its own rows.  Image b's detections are its first counts[b] rows; the rows past them are not written."""
    NC = logits.shape[1]
    assert logits.shape[0] % B == 0
    R = logits.shape[0] // B
    if R > 1024:
        raise ValueError("postprocess: %d proposals; the per-class sort takes at most 1024 per image "
                         "(MODEL.RPN.POST_NMS_TOP_N_TEST)" % R)
    cap = (NC - 1) * R
    dev = logits.device
    ob = torch.empty((B, cap, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((B, cap), dtype=torch.float32, device=dev)
    ol = torch.empty((B, cap), dtype=torch.int64, device=dev)
    oc = torch.zeros((B,), dtype=torch.int32, device=dev)
    nb = _lib.load().mega_postprocess_batched_workspace_bytes(B, R, NC)
    ws = _ws(nb, dev)
    assert logits.dtype == torch.float32 and deltas.dtype == torch.float32 and props.dtype == torch.float32
    assert logits.is_contiguous() and deltas.is_contiguous() and props.is_contiguous()
    assert deltas.shape == (B * R, NC * 4) and props.shape == (B * R, 4)
    wx, wy, ww, wh = weights
    if nprop is not None:      # device i32 [B]: the valid proposal rows of each image (rows past it are ignored)
        assert nprop.dtype == torch.int32 and nprop.numel() == B and nprop.is_contiguous()
    _call("mega_postprocess_batched", logits, deltas, props, nprop, B, R, NC, wx, wy, ww, wh, float(im_w), float(im_h),
          float(score_thresh), float(nms_thresh), int(strict_gt), int(max_det), ob, os_, ol, oc, None, ws, nb,
          prof=("postprocess", 0.0, (logits.numel() + deltas.numel()) * 4))
    return ob, os_, ol, oc


def postprocess_candidates_batched(logits, deltas, props, B, weights, im_w, im_h, score_thresh, nprop=None):
    """The candidates of B images of R = rows / B proposals each (include/mega_hip.h mega_postprocess_candidates_batched):
    (boxes [B,NC-1,R,4], scores [B,NC-1,R]) -- class j + 1, proposal row r; the score is -1 where it is not > score_thresh
    or r >= nprop[b].  Every slot is written; the box of a slot whose score is -1 is the decode of whatever that row holds
    (NaN for a padding row) and no part of the result."""
    NC = logits.shape[1]
    assert logits.shape[0] % B == 0
    R = logits.shape[0] // B
    assert logits.dtype == torch.float32 and deltas.dtype == torch.float32 and props.dtype == torch.float32
    assert logits.is_contiguous() and deltas.is_contiguous() and props.is_contiguous()
    assert deltas.shape == (B * R, NC * 4) and props.shape == (B * R, 4)
    if nprop is not None:
        assert nprop.dtype == torch.int32 and nprop.numel() == B and nprop.is_contiguous()
    dev = logits.device
    cb = torch.empty((B, NC - 1, R, 4), dtype=torch.float32, device=dev)
    cs = torch.empty((B, NC - 1, R), dtype=torch.float32, device=dev)
    wx, wy, ww, wh = weights
    _call("mega_postprocess_candidates_batched", logits, deltas, props, nprop, B, R, NC, wx, wy, ww, wh, float(im_w),
          float(im_h), float(score_thresh), cb, cs, prof=("postprocess", 0.0, (logits.numel() + deltas.numel()) * 4))
    return cb, cs


def postprocess_candidates(logits, deltas, props, nprop, weights, im_w, im_h, score_thresh):
    """One image: (boxes [NC-1,R,4], scores [NC-1,R]) as postprocess_candidates_batched."""
    if nprop is not None:
        nprop = nprop.reshape(1)
    cb, cs = postprocess_candidates_batched(logits, deltas, props, 1, weights, im_w, im_h, score_thresh, nprop=nprop)
    return cb[0], cs[0]


BBOX_AUG_MAX_VIEWS = 16
BBOX_AUG_MAX_ROWS = 8192


def _merge_setup(name, ws_bytes, cboxes, cscores, view_sizes, view_flips):
    """What bbox_aug_merge and soft_merge share: shape and limit checks (ValueError texts start with `name`), outputs,
    workspace (ws_bytes: the entry point's *_workspace_bytes) and the views as ctypes int arrays (they pass as the void
    pointers) -> F, K, R, NC, (boxes, scores, labels, counts), [view_w, view_h, view_flip], ws, its bytes."""
    K, F, C1, R = cscores.shape
    if K != len(view_sizes) or K != len(view_flips):
        raise ValueError("%s: %d views of candidates, %d sizes, %d flips" % (name, K, len(view_sizes), len(view_flips)))
    if K > BBOX_AUG_MAX_VIEWS or K * R > BBOX_AUG_MAX_ROWS:
        raise ValueError("%s: %d views x %d rows per class; the merge takes at most %d views and %d rows "
                         "per (frame, class)" % (name, K, R, BBOX_AUG_MAX_VIEWS, BBOX_AUG_MAX_ROWS))
    assert cboxes.shape == (K, F, C1, R, 4) and cboxes.dtype == torch.float32 and cscores.dtype == torch.float32
    assert cboxes.is_contiguous() and cscores.is_contiguous()
    dev = cboxes.device
    cap = C1 * K * R
    outs = (torch.empty((F, cap, 4), dtype=torch.float32, device=dev), torch.empty((F, cap), dtype=torch.float32, device=dev),
            torch.empty((F, cap), dtype=torch.int64, device=dev), torch.zeros((F,), dtype=torch.int32, device=dev))
    nb = ws_bytes(F, K, R, C1 + 1)
    arr = ctypes.c_int * K
    views = [arr(*[int(s[0]) for s in view_sizes]), arr(*[int(s[1]) for s in view_sizes]),
             arr(*[1 if f else 0 for f in view_flips])]
    return F, K, R, C1 + 1, outs, views, _ws(nb, dev), nb


def bbox_aug_merge(cboxes, cscores, view_sizes, view_flips, score_thresh, nms_thresh, max_det, strict_gt=True):
    """Test-time box augmentation merge of F frames x K views (include/mega_hip.h mega_bbox_aug_merge).
    cboxes [K,F,NC-1,R,4] / cscores [K,F,NC-1,R] f32 (the candidates of every view, each in its own image), view_sizes
    [(w, h)] x K (view 0 = the identity view, whose image the results are in), view_flips [bool] x K.  Returns
    (boxes [F,cap,4], scores [F,cap], labels [F,cap] i64, counts [F] i32 device), cap = (NC-1) * K * R: frame f's
    detections are the first counts[f] rows; the rows past them are not written.  Raises ValueError beyond K = 16 views or
    K * R = 8192 rows per class."""
    F, K, R, NC, (ob, os_, ol, oc), (vw, vh, vf), ws, nb = _merge_setup(
        "bbox_aug_merge", _lib.load().mega_bbox_aug_merge_workspace_bytes, cboxes, cscores, view_sizes, view_flips)
    _call("mega_bbox_aug_merge", cboxes, cscores, F, K, R, NC, vw, vh, vf, float(score_thresh), float(nms_thresh),
          int(strict_gt), int(max_det), ob, os_, ol, oc, ws, nb,
          prof=("bbox_aug_merge", 0.0, (cboxes.numel() + cscores.numel()) * 4))
    return ob, os_, ol, oc


SOFT_NMS_METHODS = {None: 0, "linear": 1, "gaussian": 2}
BBOX_VOTE_SCORING = {"ID": 0, "AVG": 1}


def soft_merge(cboxes, cscores, view_sizes, view_flips, score_thresh, nms_thresh, max_det, strict_gt=True, soft_method=None,
               sigma=0.5, vote=False, vote_thresh=0.8, vote_scoring="ID"):
    """bbox_aug_merge with soft-NMS and / or box voting as the final filter (include/mega_hip.h mega_soft_merge; the
    definition is soft_nms.py's).  soft_method None | "linear" | "gaussian"; vote_scoring "ID" | "AVG".  Inputs, outputs
    and limits as bbox_aug_merge; with soft_method None and vote False the result is bbox_aug_merge's, bit for bit."""
    if soft_method not in SOFT_NMS_METHODS:
        raise ValueError("soft_merge: soft_method %r, not None, 'linear' or 'gaussian'" % (soft_method,))
    if vote_scoring not in BBOX_VOTE_SCORING:
        raise ValueError("soft_merge: vote_scoring %r, not 'ID' or 'AVG'" % (vote_scoring,))
    if not float(sigma) > 0:
        raise ValueError("soft_merge: sigma = %r must be > 0" % (sigma,))
    if not 0 < float(vote_thresh) <= 1:
        raise ValueError("soft_merge: vote_thresh = %r must be in (0, 1]" % (vote_thresh,))
    F, K, R, NC, (ob, os_, ol, oc), (vw, vh, vf), ws, nb = _merge_setup(
        "soft_merge", _lib.load().mega_soft_merge_workspace_bytes, cboxes, cscores, view_sizes, view_flips)
    _call("mega_soft_merge", cboxes, cscores, F, K, R, NC, vw, vh, vf, float(score_thresh), float(nms_thresh),
          int(strict_gt), SOFT_NMS_METHODS[soft_method], float(sigma), 1 if vote else 0, float(vote_thresh),
          BBOX_VOTE_SCORING[vote_scoring], int(max_det), ob, os_, ol, oc, ws, nb,
          prof=("soft_merge", 0.0, (cboxes.numel() + cscores.numel()) * 4))
    return ob, os_, ol, oc


# ------------------------------------------------------------------------------------------------ relation module
def position_logits(rois_q, rois_k, wg_t, bg, dim_mat, precise=True, tiled=False):
    """-> [16, Nq, ldp] f32 with ldp = roundup(Nk, 32).  precise=False: fast sin/cos (bf16 mode).
    tiled=True (bf16 mode only): -> bf16 [16, ceil(Nk/32), Nq, 32] in the attention kernel's tile order (half the
    bytes; relation_attention recognises it by its dtype).
    Only the logits of the keys below Nk are written: the pad columns Nk .. ldp-1 of the rows, and the pad-key slots of the
    last tile, hold whatever the allocator's block held (NaN included).  The attention kernels never let a pad key's logit
    reach the softmax."""
    Nq, Nk = rois_q.shape[0], rois_k.shape[0]
    if tiled:        # one problem of the batched launch (the tile-ordered kernel has no other launch form)
        assert not precise, "the tile-ordered position logits are bf16 / f16"
        if Nq == 0 or Nk == 0:      # nothing to compute (the C entry returns before any launch; a batch has no empty problems)
            return torch.empty((16, (Nk + 31) // 32, Nq, 32), dtype=torch.bfloat16 if tiled is True else tiled, device=rois_q.device)
        return position_logits_batched([rois_q], [rois_k], wg_t, bg, dim_mat, precise=False, tiled=tiled)[0]
    ldp = (Nk + 31) // 32 * 32
    out = torch.empty((16, Nq, ldp), dtype=torch.float32, device=rois_q.device)
    _call("mega_position_logits", rois_q.contiguous(), rois_k.contiguous(), wg_t, bg, dim_mat, out, Nq, Nk, ldp,
          int(precise), prof=("pos_logits", 2.0 * Nq * Nk * 1024, 16.0 * Nq * ldp * 4))
    return out


def relation_attention(q, k, vt, Nk, pos=None, resid=None, bias_v=None, groups=16):
    """q [Nq,G*64] (u folded in), k [Nk,G*64], vt [G*64, ldv] key-contiguous projected V -> [Nq, G*64].
    One problem of relation_attention_batched: every attention kernel has one launch form, a batch."""
    if q.shape[0] == 0:             # no query rows: nothing to launch (a batch has no empty problems)
        return torch.empty((0, groups * 64), dtype=q.dtype if resid is None else resid.dtype, device=q.device)
    return relation_attention_batched([{"q": q, "k": k, "vt": vt, "Nk": Nk, "pos": pos, "resid": resid,
                                        "bias_v": bias_v}], groups)[0]


_ATT_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}      # attention kernel family names (bench.py's per-family roofline)
_MAX_BATCHED = 20    # problems per batched position-logit / attention launch (POS_MAXB / ATTN_MAXB in relation.hip)


def _even_chunks(n, cap):
    """problems per launch when n problems go out in launches of at most `cap`: as even as possible (20 -> 10 + 10, not
    16 + 4: a 4-problem launch leaves most of the chip idle)"""
    launches = -(-n // cap)
    return -(-n // launches) if launches else cap


# the descriptor structs of the batched / segmented entry points, as include/mega_hip.h declares them
_AttnDesc, _PosDesc, _CopySeg = (_lib.STRUCTS[n] for n in ("mega_attn_desc", "mega_pos_desc", "mega_copy_seg"))


def position_logits_batched(rois_qs, rois_ks, wg_t, bg, dim_mat, precise=True, tiled=False):
    """position_logits for several (query boxes, key boxes) problems; the tile-ordered bf16 form (bf16 mode) runs as
    ONE launch per 20 problems, the f32 forms fall back to one call per problem."""
    if not tiled:
        return [position_logits(a, b, wg_t, bg, dim_mat, precise=precise, tiled=False) for a, b in zip(rois_qs, rois_ks)]
    tdt = torch.bfloat16 if tiled is True else tiled
    assert tdt in _HALF, "the tile-ordered position logits are bf16 / f16"
    _gpu(*rois_qs, *rois_ks)      # (they reach the kernel through the descriptors, not through _call)
    outs, keep = [], []
    for a, b in zip(rois_qs, rois_ks):
        a, b = a.contiguous(), b.contiguous()
        keep.append((a, b))
        outs.append(torch.empty((16, (b.shape[0] + 31) // 32, a.shape[0], 32), dtype=tdt, device=a.device))
    per = _even_chunks(len(outs), _MAX_BATCHED)
    for o in range(0, len(outs), per):
        n = min(per, len(outs) - o)
        arr = (_PosDesc * n)()
        for i in range(n):
            a, b = keep[o + i]
            arr[i].rois_q, arr[i].rois_k, arr[i].out = a.data_ptr(), b.data_ptr(), outs[o + i].data_ptr()
            arr[i].Nq, arr[i].Nk = a.shape[0], b.shape[0]
        _call("mega_position_logits_tiled_batched_dt", ctypes.addressof(arr), n, wg_t, bg, dim_mat, _DT[tdt],
              prof=("pos_logits", sum(2.0 * arr[i].Nq * arr[i].Nk * 1024 for i in range(n)),
                    sum(outs[o + i].numel() * 2.0 for i in range(n))))
    return outs


def relation_attention_batched(items, groups=16):
    """relation_attention for a list of independent problems, each a dict(q, k, vt, Nk, pos, resid, bias_v), in ONE launch
    per 20 problems (+ one combine launch).  A problem's bits do not depend on what it is batched with."""
    if not items:
        return []
    dt = items[0]["q"].dtype
    # stream dtype: the residual's (the head's f32 activation stream over bf16 operands), else the operands'
    r0 = items[0].get("resid")
    sdt = dt if r0 is None else r0.dtype
    io_f32 = int(sdt == torch.float32 and dt != torch.float32)
    outs, wss = [], []
    # one output buffer, the problems' row blocks in order (the next batched GEMM reads it without a concatenation)
    out_all = torch.empty((sum(it["q"].shape[0] for it in items), groups * 64), dtype=sdt, device=items[0]["q"].device)
    o = 0
    for it in items:
        q, k, vt, pos = it["q"], it["k"], it["vt"], it.get("pos")
        _gpu(q, k, vt, pos, it.get("resid"), it.get("bias_v"))
        # q / k / resid: row blocks (or column-complete views) of wider buffers are fine -- unit column stride, the row
        # stride is what the kernel gets as the leading dimension, 16-byte aligned rows
        resid = it.get("resid")
        assert resid is None or resid.dtype == sdt
        for t_ in (q, k, resid):
            assert t_ is None or (t_.dtype in (dt, sdt) and t_.stride(1) == 1 and t_.data_ptr() % 16 == 0 and
                                  (t_.stride(0) * t_.element_size()) % 16 == 0)
        assert q.dtype == k.dtype == vt.dtype == dt
        # vt: [G*64, >= ceil32(Nk)] with unit column stride; a column block of a wider matrix is fine (16-B aligned).
        # With a second key segment (k2 / vt2 / N1) the blocks are read in place at element alignment: no such constraint.
        if it.get("k2") is None:
            assert vt.stride(1) == 1 and vt.shape[1] >= (it["Nk"] + 31) // 32 * 32 and vt.data_ptr() % 16 == 0 and \
                (vt.stride(0) * vt.element_size()) % 16 == 0
            assert k.shape[0] >= it["Nk"]
        else:
            _gpu(it["k2"], it["vt2"])
            assert it["k2"].data_ptr() % 16 == 0 and (vt.stride(0) * vt.element_size()) % 16 == 0
        assert (pos is None) == (items[0].get("pos") is None) and (pos is None or pos.dtype == items[0]["pos"].dtype)
        outs.append(out_all[o:o + q.shape[0]])
        o += q.shape[0]
        nb = _lib.load().mega_relation_attention_workspace_bytes(q.shape[0], it["Nk"], groups)
        wss.append(_ws(nb, q.device) if nb else None)
    per = _even_chunks(len(items), _MAX_BATCHED)
    for o in range(0, len(items), per):
        n = min(per, len(items) - o)
        arr = (_AttnDesc * n)()
        fl = by = 0.0
        for i in range(n):
            it, d = items[o + i], arr[i]
            q, k, vt, pos, resid = it["q"], it["k"], it["vt"], it.get("pos"), it.get("resid")
            Nq, Nk = q.shape[0], it["Nk"]
            d.q, d.k, d.vt, d.out = q.data_ptr(), k.data_ptr(), vt.data_ptr(), outs[o + i].data_ptr()
            d.ldq, d.ldk, d.ldv, d.ldo, d.Nq, d.Nk = q.stride(0), k.stride(0), vt.stride(0), groups * 64, Nq, Nk
            k2, vt2 = it.get("k2"), it.get("vt2")
            if k2 is not None:          # second key segment (keys N1 .. Nk-1), read where it lies
                N1 = it["N1"]
                assert 0 < N1 < Nk and k.shape[0] >= N1 and k2.shape[0] == Nk - N1 and vt2.shape[1] >= Nk - N1
                assert k2.dtype == k.dtype and vt2.dtype == vt.dtype and k2.stride(0) == k.stride(0)
                assert k2.stride(1) == 1 and vt2.stride(1) == 1 and vt.shape[1] >= N1
                d.nk1, d.k2, d.vt2, d.ldv2 = N1, k2.data_ptr(), vt2.data_ptr(), vt2.stride(0)
            d.resid, d.ldr = _ptr(resid), 0 if resid is None else resid.stride(0)
            d.io_f32 = io_f32
            d.bias_v = _ptr(it.get("bias_v"))
            if pos is not None and pos.dtype in _HALF:
                assert pos.dtype == dt and pos.is_contiguous() and tuple(pos.shape) == (groups, (Nk + 31) // 32, Nq, 32)
                d.pos_tiled = pos.data_ptr()
            elif pos is not None:
                d.pos, d.ldp = pos.data_ptr(), pos.shape[2]
            w = wss[o + i]
            d.ws, d.ws_bytes = _ptr(w), 0 if w is None else w.numel()
            fl += 4.0 * Nq * Nk * 64 * groups
            by += (q.numel() + k.numel() + vt.numel()) * q.element_size() + outs[o + i].numel() * outs[o + i].element_size() + \
                (0 if pos is None else pos.numel() * pos.element_size())
        _call("mega_relation_attention_batched", ctypes.addressof(arr), n, groups, 1.0 / math.sqrt(64.0), _DT[dt],
              prof=("attention_" + _ATT_NAME.get(dt, "f32"), fl, by))
    return outs


def copy_blocks(pairs):
    """[(dst, src)]: 2-D tensors of equal shape / dtype with unit column stride (row / column blocks of wider buffers
    are fine) -> all copies in ONE launch (mega_copy_segments).  Nothing outside the destination blocks is written."""
    pairs = [(d, s_) for d, s_ in pairs if d.numel() > 0]
    if not pairs:
        return
    arr = (_CopySeg * len(pairs))()
    nbytes = 0
    for i, (d, s_) in enumerate(pairs):
        _gpu(d, s_)
        assert d.dim() == 2 and d.shape == s_.shape and d.dtype == s_.dtype, (d.shape, s_.shape, d.dtype, s_.dtype)
        assert (d.shape[1] == 1 or (d.stride(1) == 1 and s_.stride(1) == 1))
        es = d.element_size()
        arr[i].src, arr[i].dst = s_.data_ptr(), d.data_ptr()
        arr[i].src_stride, arr[i].dst_stride = s_.stride(0) * es, d.stride(0) * es
        arr[i].rows, arr[i].row_bytes = d.shape[0], d.shape[1] * es
        nbytes += 2 * d.numel() * es
    _call("mega_copy_segments", ctypes.addressof(arr), len(pairs), prof=("assemble", 0.0, nbytes))


def multi_cat(groups):
    """Several independent torch.cat calls as ONE launch: groups = [(pieces, dim)], pieces = 2-D tensors (same dtype and
    device, unit column stride, equal sizes along the other dimension) -> [torch.cat(pieces, dim) for each group], same
    bits.  The concatenations must not depend on each other's results."""
    outs, pairs = [], []
    for pieces, dim in groups:
        pieces = list(pieces)
        p0 = pieces[0]
        if dim == 0:
            out = torch.empty((sum(p.shape[0] for p in pieces), p0.shape[1]), dtype=p0.dtype, device=p0.device)
        else:
            out = torch.empty((p0.shape[0], sum(p.shape[1] for p in pieces)), dtype=p0.dtype, device=p0.device)
        o = 0
        for p in pieces:
            assert p.dtype == p0.dtype and p.shape[1 - dim] == p0.shape[1 - dim]
            n = p.shape[dim]
            pairs.append((out.narrow(dim, o, n), p))
            o += n
        outs.append(out)
    copy_blocks(pairs)
    return outs


def cat_rows_cast_bf16(pieces, dtype=torch.bfloat16):
    """torch.cat(pieces, 0).to(dtype) (bfloat16 / float16) for f32 row blocks [n_i, K] (K % 8 == 0, unit column stride) in
    ONE launch that never writes the f32 concatenation: the K / V sources of the relation modules under an f32 activation
    stream."""
    pieces = [p for p in pieces if p.shape[0] > 0]
    K = pieces[0].shape[1]
    assert dtype in _HALF
    out = torch.empty((sum(p.shape[0] for p in pieces), K), dtype=dtype, device=pieces[0].device)
    arr = (_CopySeg * len(pieces))()
    o, nbytes = 0, 0
    for i, p in enumerate(pieces):
        _gpu(p)
        assert p.dtype == torch.float32 and p.dim() == 2 and p.shape[1] == K and K % 8 == 0 and p.stride(1) == 1
        d = out[o:o + p.shape[0]]
        arr[i].src, arr[i].dst = p.data_ptr(), d.data_ptr()
        arr[i].src_stride, arr[i].dst_stride = p.stride(0) * 4, K * 2
        arr[i].rows, arr[i].row_bytes = p.shape[0], K * 4
        o += p.shape[0]
        nbytes += p.numel() * 6
    _call("mega_copy_cast_segments_dt", ctypes.addressof(arr), len(pieces), _DT[dtype], prof=("assemble", 0.0, nbytes))
    return out


def resize_bilinear_u8(frames_u8, out_hw, tables):
    """uint8 [N,Hi,Wi,3] -> [N,Ho,Wo,3], Pillow-exact BILINEAR.  tables = feed.ResizeTables (device coefficient tables)."""
    N, Hi, Wi, C = frames_u8.shape
    Ho, Wo = out_hw
    assert C == 3 and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
    assert tables.in_hw == (Hi, Wi) and tables.out_hw == (Ho, Wo)
    out = torch.empty((N, Ho, Wo, 3), dtype=torch.uint8, device=frames_u8.device)
    tmp = torch.empty((N, Hi, Wo, 3), dtype=torch.uint8, device=frames_u8.device) if (Hi != Ho and Wi != Wo) else None
    _call("mega_resize_bilinear_u8", frames_u8, out, tmp, N, Hi, Wi, Ho, Wo, tables.bounds_h, tables.coef_h, tables.ksize_h,
          tables.bounds_v, tables.coef_v, tables.ksize_v, prof=("resize", 0.0, frames_u8.numel() + out.numel() * 3))
    return out


def resize_bilinear_u8_flip(frames_u8, out_hw, tables, hflip=True):
    """resize_bilinear_u8 followed by a left-right mirror (PIL resize(BILINEAR).transpose(FLIP_LEFT_RIGHT)), the mirror
    written by the last pass.  tables may be None when out_hw is the input size (the mirror alone)."""
    N, Hi, Wi, C = frames_u8.shape
    Ho, Wo = out_hw
    assert C == 3 and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
    if (Ho, Wo) != (Hi, Wi):
        assert tables is not None and tables.in_hw == (Hi, Wi) and tables.out_hw == (Ho, Wo)
    out = torch.empty((N, Ho, Wo, 3), dtype=torch.uint8, device=frames_u8.device)
    tmp = torch.empty((N, Hi, Wo, 3), dtype=torch.uint8, device=frames_u8.device) if (Hi != Ho and Wi != Wo) else None
    t = tables
    _call("mega_resize_bilinear_u8_flip", frames_u8, out, tmp, N, Hi, Wi, Ho, Wo, t.bounds_h if t else None,
          t.coef_h if t else None, t.ksize_h if t else 0, t.bounds_v if t else None, t.coef_v if t else None,
          t.ksize_v if t else 0, int(bool(hflip)),
          prof=("resize", 0.0, frames_u8.numel() + out.numel() * 3))
    return out


def preprocess_frames(frames_u8, mean, to_bgr=True, out=None):
    """uint8 [N,H,W,3] RGB -> f32 [N,3,H,W] (BGR*255 - mean); out: optional contiguous f32 [N,3,H,W] to write into."""
    N, H, W, C = frames_u8.shape
    assert C == 3 and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
    if out is None:
        out = torch.empty((N, 3, H, W), dtype=torch.float32, device=frames_u8.device)
    else:
        assert out.shape == (N, 3, H, W) and out.dtype == torch.float32 and out.is_contiguous()
    _call("mega_preprocess_frames", frames_u8, out, N, H, W, float(mean[0]), float(mean[1]), float(mean[2]), int(to_bgr),
          prof=("preprocess", 0.0, frames_u8.numel() * 5))
    return out


def cast_half(x, dtype):
    """f32 -> bf16 / f16 copy (round to nearest even) of a contiguous tensor; an input of that dtype is returned as it is."""
    if x.dtype == dtype:
        return x
    assert x.dtype == torch.float32 and x.is_contiguous() and dtype in _HALF
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _call("mega_cast_f32_to_half", x, out, x.numel(), _DT[dtype], prof=("assemble", 0.0, x.numel() * 6.0))
    return out


def cast_bf16(x):
    return cast_half(x, torch.bfloat16)


def split_bf16x3(x):
    """f32 [M,K] -> bf16 [M,3K] = [hi | lo | hi] (hi = bf16(x), lo = bf16(x - hi)): A operand of a split-precision bf16
    GEMM against weights packed by split_weight_bf16x3."""
    M, K = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and K % 8 == 0
    out = torch.empty((M, 3 * K), dtype=torch.bfloat16, device=x.device)
    _call("mega_split_f32_to_bf16x3", x, out, M, K, prof=("assemble", 0.0, x.numel() * 10.0))
    return out


def split_weight_bf16x3(w32):
    """f32 [N,K] -> bf16 [N,3K] = [Wh | Wh | Wl]: with split_bf16x3(x) as the other operand, the K = 3K contraction is
    x_hi.Wh + x_lo.Wh + x_hi.Wl = x.W to ~2^-16 (host-side packing, once per model)."""
    wh = w32.to(torch.bfloat16)
    wl = (w32 - wh.float()).to(torch.bfloat16)
    return torch.cat([wh, wh, wl], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------ split-precision planes
class Planes(object):
    """An f32 activation [..., C] held as bf16 [..., 2C] = [hi | lo] planes (hi = bf16(x), lo = bf16(x - hi); x = hi + lo to
    ~2^-17): what the split-precision ("bf16 x 3") frame stage and the wide residual stream of the bf16 mode keep in HBM.
    `t` is the contiguous bf16 tensor, `C` the logical channel count."""
    __slots__ = ("t", "C")

    def __init__(self, t, C):
        assert t.dtype in _HALF and t.shape[-1] == 2 * C and t.is_contiguous()     # (float16 pairs: the fp16 two-pass mode)
        self.t, self.C = t, C

    @property
    def dtype(self):
        return self.t.dtype

    @property
    def shape(self):
        return tuple(self.t.shape[:-1]) + (self.C,)

    @property
    def device(self):
        return self.t.device

    def float(self):
        """hi + lo as an f32 tensor (torch ops; tests and seams only)"""
        return self.t[..., :self.C].float() + self.t[..., self.C:].float()

    def hi(self):
        return self.t[..., :self.C]


def split_planes(x, dtype=torch.bfloat16):
    """f32 [..., C] (contiguous, C % 8 == 0) -> Planes of `dtype` pairs (one launch)."""
    C = x.shape[-1]
    assert x.dtype == torch.float32 and x.is_contiguous() and C % 8 == 0 and dtype in _HALF
    out = torch.empty(tuple(x.shape[:-1]) + (2 * C,), dtype=dtype, device=x.device)
    _call("mega_split_f32_to_planes_dt", x, out, x.numel() // C, C, _DT[dtype], prof=("assemble", 0.0, x.numel() * 8.0))
    return Planes(out, C)


def split_conv_weight_h2(w_ohwi):
    """f32 conv weight [Cout,R,S,C] (OHWI) -> float16 [Cout,R,S,2C] = [W | W] per tap, W rounded to fp16 once: the operand of
    conv2d_sp(operands="h2") -- against fp16 [hi | lo] planes the K = 2C contraction is x_hi.W + x_lo.W (the two-pass fp16 mode)."""
    w = w_ohwi.float().to(torch.float16)
    return torch.cat([w, w], dim=-1).contiguous()


def split_conv_weight_x3(w_ohwi):
    """f32 conv weight [Cout,R,S,C] (OHWI) -> bf16 [Cout,R,S,3C] = [Wh | Wh | Wl] per tap: the operand of conv2d_sp(operands="x3")
    (host-side packing, once per model)."""
    w32 = w_ohwi.float()
    wh = w32.to(torch.bfloat16)
    wl = (w32 - wh.float()).to(torch.bfloat16)
    return torch.cat([wh, wh, wl], dim=-1).contiguous()


# operand form of conv2d_sp / linear_sp -> (K multiple of the weight, dtype of planes and weight, K wraps back to the hi plane):
#   "x3"  planes read as [hi | lo | hi] against w = split_conv_weight_x3(W) [Cout,R,S,3C]: x.W to ~2^-16, f32 accumulation
#   "h2"  the two-pass fp16 form: float16 planes read as [hi | lo] (no wrap) against w = split_conv_weight_h2(W) [Cout,R,S,2C]
#   "hi"  only the hi plane is read, against plain bf16 w [Cout,R,S,C] (bf16 compute over a wide residual stream)
_SP_OPERANDS = {"x3": (3, torch.bfloat16, True), "h2": (2, torch.float16, False), "hi": (1, torch.bfloat16, False)}


def _sp_operands(operands):
    if operands not in _SP_OPERANDS:
        raise ValueError("operands must be one of %s, not %r" % (sorted(_SP_OPERANDS), operands))
    return _SP_OPERANDS[operands]


def conv2d_sp(x, w, scale=None, bias=None, residual=None, stride=1, pad=0, dil=1, relu=False, out_mode="planes",
              operands="x3", out=None):
    """conv + FrozenBN (+ residual) + activation on split-precision planes (mega_conv2d_nhwc_sp_dt, igemm8 SP kernels).
    x: Planes [N,H,W,C]; w: the weight in the form `operands` names (_SP_OPERANDS).  residual: Planes [N,Ho,Wo,Cout]
    (hi + lo added in f32).  out_mode: "planes" -> Planes, "f32" -> f32 tensor, "bf16" -> bf16 tensor  [N,Ho,Wo,Cout]."""
    kmul, pdt, kwrap = _sp_operands(operands)
    assert residual is None or isinstance(residual, Planes)
    if not isinstance(x, Planes):      # a plain bf16 tensor as the input (pixel stride C): operands "hi" only
        assert x.dtype == torch.bfloat16 and x.is_contiguous() and operands == "hi"
        xt, ldi = x, x.shape[-1]
    else:
        xt, ldi = x.t, 2 * x.C
    assert xt.dtype == pdt and (residual is None or residual.t.dtype == pdt)
    N, H, W, C = x.shape
    Cout, R, S, Cw = w.shape
    assert Cw == kmul * C and w.dtype == pdt and w.is_contiguous() and C % 64 == 0 and Cout % 8 == 0
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    mode = {"bf16": 0, "planes": 1, "f32": 2}[out_mode]
    ldo = 0
    if out is not None:      # caller's [N*Ho*Wo, ldo >= Cout] buffer (plain output modes): row stride = its width
        assert mode != 1 and out.dim() == 2 and out.shape[0] == N * Ho * Wo and out.shape[1] >= Cout and out.is_contiguous()
        assert out.dtype == (torch.float32 if mode == 2 else pdt)
        ldo = out.shape[1]
    elif mode == 1:
        out = torch.empty((N, Ho, Wo, 2 * Cout), dtype=pdt, device=x.device)
    else:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32 if mode == 2 else pdt, device=x.device)
    if residual is not None:
        assert residual.shape == (N, Ho, Wo, Cout)
    for v in (scale, bias):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout and v.is_contiguous())
    if max(xt.numel(), w.numel(), out.numel() * (2 if mode == 2 else 1)) * 2 >= 0x7FF00000:
        raise ValueError("conv2d_sp: an operand of 2 GiB or more; the kernels use 32-bit buffer offsets: lower the "
                         "frame-stage batch (ClipEngine steps_per_batch) or split the call over M")
    K = R * S * Cw
    M = N * Ho * Wo
    prof = None
    if _PROF is not None:
        prof = ("igemm8_sp_" + operands, 2.0 * M * Cout * K,
                xt.numel() * (2.0 if operands != "hi" or xt is x else 1.0) + w.numel() * 2.0 + out.numel() * out.element_size()
                + (0 if residual is None else residual.t.numel() * 2.0), "%dx%dx%d (%dx%d)" % (M, Cout, K, R, S))
    nb = _lib.load().mega_conv2d_nhwc_workspace_bytes(M, Cout, K) if mode == 2 and residual is None else 0
    ws = _ws(nb, x.device) if nb else None
    _call("mega_conv2d_nhwc_sp_dt", xt, ldi, 2 * C if kwrap else 0, w, scale, bias, None if residual is None else residual.t,
          0, out, ldo, mode, N, H, W, Cw, Cout, R, S, stride, pad, dil, int(relu), _DT[pdt], ws, nb, prof=prof)
    return Planes(out, Cout) if mode == 1 else out


# ------------------------------------------------------------------------------------------------ FP8 conv (f8.py)
F8 = 3      # MEGA_F8: OCP e4m3fn codes


def pack_conv_weight_f8(w_ohwi_f32):
    """f32 conv weight [Cout,R,S,Cin] (OHWI) -> (codes float8_e4m3fn [Cout,R,S,Cin], sw f32 [Cout]): one scale per output
    channel, sw[o] = absmax(w[o]) / 448 (1 for an all-zero channel), codes = f8.quantize(w[o], 1 / sw[o])."""
    w = w_ohwi_f32.float().contiguous()
    sw = f8.weight_scales(w)
    return f8.quantize(w, (1.0 / sw).view(-1, 1, 1, 1)).contiguous(), sw.contiguous()


def f8_conv_admitted(N, H, W, Cin, Cout, R, S, stride, pad, dil):
    """the shapes mega_conv2d_nhwc_f8 admits (the library's own rule, mega_conv2d_nhwc_f8_plan, says the same)"""
    geo = (R, S, pad) in ((1, 1, 0), (3, 3, 1)) and stride == 1 and dil == 1
    return bool(geo and min(N, H, W) >= 1 and Cin >= 128 and Cin % 128 == 0 and Cout >= 64 and Cout % 64 == 0
                and max(H, W) <= 1 << 20 and N * H * W <= 0x3FFFFFFF)


def conv2d_nhwc_f8(x, w_codes, scale, bias, in_scale=None, out_scale=None, pad=0, relu=False, stride=1, dil=1, out=None):
    """conv + scale / bias (+ ReLU) on FP8 operands (mega_conv2d_nhwc_f8; f8.py defines the quantisation).
    x [N,H,W,Cin]: float8_e4m3fn codes, or bfloat16 with in_scale = the tensor's scale s (quantised with 1 / s on the kernel's
    load path); w_codes [Cout,R,S,Cin] float8_e4m3fn; scale / bias f32 [Cout] (the caller folds s_in * sw * bn_scale into
    scale: f8.fold_scale).  out_scale None: bf16 output; a scale s: float8_e4m3fn output quantize(y, 1 / s).
    An unknown dtype or a shape the kernel does not admit raises ValueError before any device or library check."""
    if x.dtype not in (torch.bfloat16, f8.FP8):
        raise ValueError("conv2d_nhwc_f8: input dtype %s (bfloat16 or float8_e4m3fn)" % x.dtype)
    if w_codes.dtype != f8.FP8:
        raise ValueError("conv2d_nhwc_f8: weight dtype %s (float8_e4m3fn codes: pack_conv_weight_f8)" % w_codes.dtype)
    if x.dim() != 4 or w_codes.dim() != 4 or x.shape[3] != w_codes.shape[3]:
        raise ValueError("conv2d_nhwc_f8: x %s against w %s" % (tuple(x.shape), tuple(w_codes.shape)))
    N, H, W, Cin = x.shape
    Cout, R, S, _ = w_codes.shape
    if not f8_conv_admitted(N, H, W, Cin, Cout, R, S, stride, pad, dil):
        raise ValueError("conv2d_nhwc_f8 does not admit x %s, w %s, stride %d, pad %d, dil %d: 1x1 / pad 0 or 3x3 / pad 1, "
                         "stride 1, dil 1, Cin %% 128 == 0, Cout %% 64 == 0" % (tuple(x.shape), tuple(w_codes.shape), stride, pad, dil))
    if x.dtype == torch.bfloat16 and in_scale is None:
        raise ValueError("conv2d_nhwc_f8: a bfloat16 input needs in_scale")
    for s in (in_scale, out_scale):
        if s is not None and not (float(s) > 0.0 and float(s) < float("inf")):
            raise ValueError("conv2d_nhwc_f8: scale %r is not a positive finite number" % (s,))
    assert x.is_contiguous() and w_codes.is_contiguous()
    for v in (scale, bias):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout and v.is_contiguous())
    odt = torch.bfloat16 if out_scale is None else f8.FP8
    if out is None:
        out = torch.empty((N, H, W, Cout), dtype=odt, device=x.device)
    else:
        assert out.dtype == odt and out.shape == (N, H, W, Cout) and out.is_contiguous()
    prof = None
    if _PROF is not None:
        prof = ("igemm_f8_%s_%s" % ("bf16in" if x.dtype == torch.bfloat16 else "f8in", "f8out" if out_scale is not None else "bf16out"),
                2.0 * N * H * W * Cout * R * S * Cin,
                x.numel() * x.element_size() + w_codes.numel() + out.numel() * out.element_size(),
                "%dx%dx%d (%dx%d)" % (N * H * W, Cout, R * S * Cin, R, S))
    _call("mega_conv2d_nhwc_f8", x, BF16 if x.dtype == torch.bfloat16 else F8, 1.0 if in_scale is None else f8.inv_scale(in_scale),
          w_codes, scale, bias, out, BF16 if out_scale is None else F8, 1.0 if out_scale is None else f8.inv_scale(out_scale),
          N, H, W, Cin, Cout, R, S, stride, pad, dil, int(bool(relu)), prof=prof)
    return out


class X3Weight(object):
    """An f32 linear weight [Nout, K] as the split-precision operand [Wh | Wh | Wl] (bf16 [Nout, 3K]).  ops.linear /
    ops.linear_transposed take it in place of the f32 matrix and run x.W on the bf16 matrix cores to ~2^-16 with f32
    accumulation (the aggregation head's projections and stage FCs in conv_mode "x3").  `dtype` reports float32: callers
    that ask the weight for the dtype of its operands hand over f32 activations."""
    dtype = torch.float32

    def __init__(self, w32, device):
        w32 = w32.detach().float()
        self.shape = tuple(w32.shape)
        self.w3 = split_conv_weight_x3(w32.contiguous().view(w32.shape[0], 1, 1, w32.shape[1])).view(w32.shape[0], -1).to(device)
        self.device = self.w3.device


def linear_transposed_x3(w, x, ld):
    """linear_transposed for an X3Weight: out[n][m] = sum_k W[n][k] x[m][k] as f32 [Nout, ld], pad columns zero.  The weight
    rows are the GEMM's A operand ([Wh | Wh | Wl], plain bf16, K x 3), the activations its B operand as [xh | xl | xh]
    (ops.split_bf16x3; rows padded with zeros to a multiple of 8: the SP kernels store whole 16-byte vectors along m)."""
    Nout, K = w.shape
    M = x.shape[0]
    assert x.dtype == torch.float32 and x.shape[1] == K and ld >= (M + 7) // 8 * 8
    M8 = (M + 7) // 8 * 8
    xs = torch.empty((M8, 3 * K), dtype=torch.bfloat16, device=x.device)
    if M8 > M:
        xs[M:].zero_()
    _call("mega_split_f32_to_bf16x3", x.contiguous(), xs, M, K)
    out = torch.empty((Nout, ld), dtype=torch.float32, device=x.device)
    if ld > M8:
        out[:, M8:].zero_()
    conv2d_sp(w.w3.view(Nout, 1, 1, 3 * K), xs.view(M8, 1, 1, 3 * K), out_mode="f32", operands="hi", out=out)
    return out


def linear_sp(x, w3, bias=None, relu=False, operands="x3"):
    """x: Planes [M,K]; w3 = split_conv_weight_x3 ("x3": x.W to ~2^-16) or split_conv_weight_h2 ("h2": float16 planes, the
    two-pass fp16 form) of [Nout,K] viewed [Nout,1,1,K] -> f32 [M,Nout]."""
    M, K = x.shape
    y = conv2d_sp(Planes(x.t.view(M, 1, 1, 2 * K), K), w3.view(w3.shape[0], 1, 1, _sp_operands(operands)[0] * K), None, bias,
                  relu=relu, out_mode="f32", operands=operands)
    return y.view(M, w3.shape[0])


def linear_transposed(w, x, ld, residual=None):
    """Returns (x @ w^T)^T (+ residual) laid out [Nout, ld] with ld >= M and the pad columns zero:
    out[n][m] = sum_k w[n][k] * x[m][k].  The weight matrix plays the GEMM 'A rows' role, so the
    projected values of one output feature are contiguous over rows m (keys).  residual: [Nout, ld] of the same dtype,
    added in the epilogue (the second pass of a split-weight projection, relation.project_v)."""
    if isinstance(w, X3Weight):
        assert residual is None
        return linear_transposed_x3(w, x, ld)
    Nout, K = w.shape
    M = x.shape[0]
    assert x.shape[1] == K and ld >= M and w.dtype == x.dtype and w.is_contiguous() and x.is_contiguous()
    assert residual is None or (residual.shape == (Nout, ld) and residual.dtype == x.dtype and residual.is_contiguous())
    # (only the pad columns are zeroed: zero-filling the whole [Nout, ld] buffer -- 155 MB at stage 0 -- before the GEMM
    #  overwrote it was 11 fill launches / 0.08 ms per 20 key frames)
    out = torch.empty((Nout, ld), dtype=x.dtype, device=x.device)
    if ld > M:
        out[:, M:].zero_()
    prof = None
    if _PROF is not None:
        prof = (_igemm_family(Nout, M, K, x.dtype), 2.0 * Nout * M * K, (w.numel() + x.numel() + out.numel()) * x.element_size())
    _call("mega_conv2d_nhwc", w, x, None, None, residual, out, Nout, 1, 1, K, M, 1, 1, 1, 0, 1, 0, ld, ld, _dt(x), _dt(x),
          prof=prof, what="mega_conv2d_nhwc(transposed)")
    return out


def dff_warp_scale(feats, flow, scale):
    """feats NHWC [H,W,C] (key frame), flow [2,H,W] f32, scale [H,W,C] -> warp(feats, flow) * scale  [H,W,C]."""
    H, W, C = feats.shape
    assert feats.is_contiguous() and flow.is_contiguous() and scale.is_contiguous()
    assert flow.dtype == torch.float32 and flow.shape == (2, H, W) and scale.shape == feats.shape and scale.dtype == feats.dtype
    out = torch.empty_like(feats)
    _call("mega_dff_warp_scale", feats, flow, scale, out, H, W, C, _dt(feats),
          prof=("dff_warp", 0.0, 6.0 * feats.numel() * feats.element_size()))
    return out


def fgfa_warp_aggregate(feats, flow, Cf, key, want_weights=False, order=None, flow_pos=None, out=None):
    """feats NHWC [T,H,W,Cf+Ce], flow [T,2,H,W] f32 -> aggregated key-frame features [H,W,Cf] (+ weights [T,H,W]).
    order (i32 [1 + T] on the device): feats is a ring of S >= T slots, order[0] = the key frame's slot, order[1 + t] = the
    slot of window position t (`key` is ignored); same bits as the call on the frames in window order.  flow is indexed by
    slot like feats ([S,2,H,W]) or, with flow_pos = the key frame's window position, by window position ([T,2,H,W]: exactly
    the window's pairs, in window order).  out: the result tensor to write ([H,W,Cf], contiguous, of feats' dtype).
    A shape the kernel cannot take (see include/mega_hip.h) raises the library's "bad argument" error before any launch."""
    S, H, W, C = feats.shape
    T = S if order is None else order.numel() - 1
    assert feats.is_contiguous() and flow.is_contiguous() and flow.dtype == torch.float32
    assert flow.shape == ((T if flow_pos is not None else S), 2, H, W) and (flow_pos is None or order is not None)
    if out is None:
        out = torch.empty((H, W, Cf), dtype=feats.dtype, device=feats.device)
    assert tuple(out.shape) == (H, W, Cf) and out.dtype == feats.dtype and out.is_contiguous()
    wts = torch.empty((T, H, W), dtype=torch.float32, device=feats.device) if want_weights else None
    prof = ("fgfa_warp", 0.0, 4.0 * feats.numel() * feats.element_size())
    if order is None:
        _call("mega_fgfa_warp_aggregate", feats, flow, out, wts, T, H, W, Cf, C - Cf, key, _dt(feats), prof=prof)
        return (out, wts) if want_weights else out
    assert order.dtype == torch.int32 and order.is_contiguous()
    if flow_pos is not None:
        _call("mega_fgfa_warp_aggregate_ring_pos", feats, flow, out, wts, T, H, W, Cf, C - Cf, order, int(flow_pos), _dt(feats),
              prof=prof)
    else:
        _call("mega_fgfa_warp_aggregate_ring", feats, flow, out, wts, T, H, W, Cf, C - Cf, order, _dt(feats), prof=prof,
              what="mega_fgfa_warp_aggregate")
    return (out, wts) if want_weights else out


def fgfa_warp_aggregate_group(feats, flow, Cf, orders, key_pos):
    """fgfa_warp_aggregate(..., order=orders[g], flow_pos=key_pos) for the G key frames of a group in ONE launch: feats ring
    [S,H,W,Cf+Ce], flow f32 [G*T,2,H,W] (window order per key frame), orders i32 [G,1+T] -> [G,H,W,Cf]; same bits per key frame."""
    S, H, W, C = feats.shape
    G, T1 = orders.shape
    T = T1 - 1
    assert feats.is_contiguous() and flow.is_contiguous() and flow.dtype == torch.float32 and tuple(flow.shape) == (G * T, 2, H, W)
    assert orders.dtype == torch.int32 and orders.is_contiguous()
    out = torch.empty((G, H, W, Cf), dtype=feats.dtype, device=feats.device)
    _call("mega_fgfa_warp_aggregate_ring_pos_batched", feats, flow, out, None, T, H, W, Cf, C - Cf, orders, int(key_pos), G,
          _dt(feats), prof=("fgfa_warp", 0.0, 4.0 * G * T * H * W * C * feats.element_size()))
    return out


def fgfa_pair_taps(refs, cur=None, order=None, dtype=torch.bfloat16):
    """FlowNetS's first-conv operand from the f32 NCHW frames in one kernel (mega_fgfa_pair_taps): refs [T,3,H,W] f32, the
    key frame `cur` [1,3,H,W] (one for all pairs) or [T,3,H,W] (one per pair), or cur=None with `order` (i32 on the device):
    the key frame is refs[order[0]] (the engine's image ring).  -> `dtype` [T, ceil(H/2) + 6, ceil(W/2), 64]:
    out[t, 3 + h, w, s * 8 + c] = avgpool2x2_ceil(cat([cur, refs[t]]))[h, w - 3 + s, c], zeros elsewhere."""
    T, C, H, W = refs.shape
    assert C == 3 and refs.dtype == torch.float32 and refs.stride(1) == H * W and refs.stride(2) == W and refs.stride(3) == 1
    assert dtype in _HALF and (cur is not None or order is not None)
    cs = 0
    if cur is not None:
        assert cur.dtype == torch.float32 and cur.shape[1:] == (3, H, W) and cur.shape[0] in (1, T)
        assert cur.stride(1) == H * W and cur.stride(2) == W and cur.stride(3) == 1
        cs = cur.stride(0) if cur.shape[0] == T else 0
    else:
        assert order.dtype == torch.int32 and order.is_contiguous()
    out = torch.empty((T, (H + 1) // 2 + 6, (W + 1) // 2, 64), dtype=dtype, device=refs.device)
    _call("mega_fgfa_pair_taps", refs, refs.stride(0), cur, cs, order, out, T, H, W, _DT[dtype],
          prof=("fgfa_pair_taps", 0.0, refs.numel() * 4.0 + out.numel() * 2.0))
    return out


def avgpool2x2_ceil(x):
    """nn.AvgPool2d(2, 2, ceil_mode=True) on NHWC."""
    N, H, W, C = x.shape
    assert x.is_contiguous()
    out = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), dtype=x.dtype, device=x.device)
    _call("mega_avgpool2x2_ceil_nhwc", x, out, N, H, W, C, _dt(x))
    return out


# ------------------------------------------------------------------------------------------------ VID evaluation
def vid_eval_match(det_box, det_label, det_off, order, ratio, gt_box, gt_label, gt_motion, gt_off, ranges, C, max_gt):
    """vid_eval.py:156-253 matching for F frames and R motion ranges (include/mega_hip.h mega_vid_eval_match).
    det_box [N,4] f32, det_label [N] i32, det_off [F+1] i64, order [N] i32, ratio [F,2] f32, gt_box [G,4] f32,
    gt_label [G] i32, gt_motion [G] f64 or None, gt_off [F+1] i64, ranges [R,3] f64 (lo, hi, empty_weight).
    -> match [R,N] u8, pred_ignore [R,N] f64, n_pos [R,C] i32 (all on the device)."""
    N, F, R = det_box.shape[0], det_off.shape[0] - 1, ranges.shape[0]
    for t, dt in ((det_box, torch.float32), (det_label, torch.int32), (det_off, torch.int64), (order, torch.int32),
                  (ratio, torch.float32), (gt_box, torch.float32), (gt_label, torch.int32), (gt_motion, torch.float64),
                  (gt_off, torch.int64), (ranges, torch.float64)):
        assert t is None or (t.dtype == dt and t.is_contiguous())
    dev = det_box.device
    match = torch.empty((R, N), dtype=torch.uint8, device=dev)
    pign = torch.empty((R, N), dtype=torch.float64, device=dev)
    n_pos = torch.empty((R, C), dtype=torch.int32, device=dev)
    _call("mega_vid_eval_match", det_box, det_label, det_off, order, ratio, gt_box, gt_label, gt_motion, gt_off, ranges, F,
          R, int(C), N, int(max_gt), match, pign, n_pos, prof=("vid_eval_match",))
    return match, pign, n_pos


def vid_eval_ap(match, pred_ignore, gorder, seg_off, n_pos):
    """vid_eval.py:255-343: per (range, class) precision / recall scans and AP over the classes' detections in global
    order gorder[seg_off[l] : seg_off[l+1]].  -> ap [R,C] f64 on the device (NaN where n_pos == 0)."""
    R, C = n_pos.shape
    N = match.shape[1]
    assert match.dtype == torch.uint8 and pred_ignore.dtype == torch.float64 and gorder.dtype == torch.int32
    assert seg_off.dtype == torch.int64 and n_pos.dtype == torch.int32 and seg_off.shape[0] == C + 1
    ap = torch.empty((R, C), dtype=torch.float64, device=match.device)
    nb = _lib.load().mega_vid_eval_workspace_bytes(N, C, R)
    ws = _ws(nb, match.device)
    _call("mega_vid_eval_ap", match, pred_ignore, gorder, seg_off, n_pos, C, R, N, ap, ws, nb, prof=("vid_eval_ap",))
    return ap


def proposal_recall_match(box, off, order, ratio, gt_box, gt_off, limits, max_limit, max_gt):
    """eval_proposals_vid's greedy matching (vid_eval.py:72-119) for F frames and nL limits in one launch
    (include/mega_hip.h mega_proposal_recall_match).  box [N,4] f32, off [F+1] i64, order [N] i32 (each frame's run in
    evaluation order), ratio [F,2] f32, gt_box [G,4] f32, gt_off [F+1] i64, limits [nL] i32 (each <= max_limit <= 1024).
    -> gt_overlap [nL,G] f32, gt_prop [nL,G] i32 (position in the frame's order, -1: unmatched), on the device."""
    N, F, G, nL = box.shape[0], off.shape[0] - 1, gt_box.shape[0], limits.shape[0]
    for t, dt in ((box, torch.float32), (off, torch.int64), (order, torch.int32), (ratio, torch.float32),
                  (gt_box, torch.float32), (gt_off, torch.int64), (limits, torch.int32)):
        assert t.dtype == dt and t.is_contiguous()
    assert box.shape == (N, 4) and order.shape == (N,) and ratio.shape == (F, 2) and gt_box.shape == (G, 4)
    assert gt_off.shape == (F + 1,)
    dev = box.device
    gt_overlap = torch.empty((nL, G), dtype=torch.float32, device=dev)
    gt_prop = torch.empty((nL, G), dtype=torch.int32, device=dev)
    _call("mega_proposal_recall_match", box, off, order, ratio, gt_box, gt_off, limits, F, nL, N, G, int(max_limit),
          int(max_gt), gt_overlap, gt_prop, prof=("proposal_recall_match",))
    return gt_overlap, gt_prop


# ------------------------------------------------------------------------------------------------ Seq-NMS
def _check_video_tensors(box, score, seg_off, tasks, F, C, pos=None):
    """The tensor checks seq_nms and link_tracks share -> (N, T)."""
    N, T = box.shape[0], tasks.shape[0]
    for t, dt in ((box, torch.float32), (score, torch.float32), (seg_off, torch.int64), (tasks, torch.int32)) + \
            (((pos, torch.int32),) if pos is not None else ()):
        assert t.dtype == dt and t.is_contiguous()
    assert box.shape == (N, 4) and score.shape == (N,) and seg_off.shape == (C * F + 1,) and tasks.shape == (T, 3)
    assert pos is None or pos.shape == (N,)
    return N, T


def seq_nms(box, score, seg_off, tasks, F, C, link_iou, nms_iou, rescore_max):
    """Seq-NMS over T (video, class) tasks (include/mega_hip.h mega_seq_nms).  box [N,4] f32, score [N] f32 sorted class-
    major then frame, seg_off [C*F+1] i64, tasks [T,3] i32 (class, first frame, frame count), longest first.
    -> keep [N] u8, new_score [N] f32 (valid where keep; the other elements are the wrapper's zeros), stats [T,2] i64
    (iterations, DP frame steps), on the device.  Every box belongs to one task, so every element of keep is written.
    Synchronises the stream (the kernel's status word)."""
    N, T = _check_video_tensors(box, score, seg_off, tasks, F, C)
    dev = box.device
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    new_score = torch.zeros(N, dtype=torch.float32, device=dev)
    stats = torch.zeros((T, 2), dtype=torch.int64, device=dev)
    nb = _lib.load().mega_seq_nms_workspace_bytes(N, C * F)
    ws = _ws(nb, dev)
    _call("mega_seq_nms", box, score, seg_off, tasks, T, int(F), int(C), N, float(link_iou), float(nms_iou),
          int(bool(rescore_max)), keep, new_score, stats, ws, nb, prof=("seq_nms",))
    return keep, new_score, stats


# ------------------------------------------------------------------------------------------------ track linking
def link_tracks(box, score, pos, seg_off, tasks, F, C, score_thresh, link_iou, max_gap, max_open):
    """Link detections into tracks over T (video, class) tasks (include/mega_hip.h mega_link_tracks).  box [N,4] f32,
    score [N] f32, pos [N] i32 sorted class-major, then frame, then descending score (equal scores: ascending position);
    seg_off [C*F+1] i64, tasks [T,3] i32 (class, first frame, frame count), longest first; max_open: a bound on a task's
    open tracks.  -> root [N] i64 (index of the track's first box in this order, -1: no track), and valid at the roots
    cnt [N] i32, sum [N] f64, mx [N] f32, on the device (the kernel writes them at the roots only: the other elements are
    the wrapper's zeros).  Synchronises the stream (the kernel's status word)."""
    N, T = _check_video_tensors(box, score, seg_off, tasks, F, C, pos)
    dev = box.device
    root = torch.full((N,), -1, dtype=torch.int64, device=dev)
    cnt = torch.zeros(N, dtype=torch.int32, device=dev)
    acc = torch.zeros(N, dtype=torch.float64, device=dev)
    mx = torch.zeros(N, dtype=torch.float32, device=dev)
    nb = _lib.load().mega_link_tracks_workspace_bytes(T, int(max_open))
    ws = _ws(max(nb, 1), dev)
    _call("mega_link_tracks", box, score, pos, seg_off, tasks, T, int(F), int(C), N, float(score_thresh), float(link_iou),
          int(max_gap), int(max_open), root, cnt, acc, mx, ws, nb, prof=("link_tracks",))
    return root, cnt, acc, mx


# ------------------------------------------------------------------------------------------------ track refinement
def refine_tracks(m_box, m_score, m_frame, m_off, o_off, slots, fill, smooth, fill_scale):
    """Fill the gap frames of K tracks and smooth their boxes (include/mega_hip.h mega_refine_tracks;
    mega/pytorch_amd/tracks.py defines it).  m_box [M,4] f32, m_score [M] f32, m_frame [M] i32: the members sorted by (video,
    track id, frame); m_off / o_off [K+1] i64: each track's members and output slots; slots: S = o_off[K], which the
    caller knows on the host.  -> per slot box [S,4] f32, score [S] f32, frame [S] i32, track [S] i32, src [S] i32 (the
    member's index, -1: filled), filled [S] u8, on the device.  Does not synchronise."""
    M, K = m_box.shape[0], m_off.shape[0] - 1
    for t, dt in ((m_box, torch.float32), (m_score, torch.float32), (m_frame, torch.int32), (m_off, torch.int64),
                  (o_off, torch.int64)):
        assert t.dtype == dt and t.is_contiguous()
    assert m_box.shape == (M, 4) and m_score.shape == (M,) and m_frame.shape == (M,) and o_off.shape == (K + 1,)
    dev = m_box.device
    S = int(slots)
    box = torch.empty((S, 4), dtype=torch.float32, device=dev)
    score = torch.empty(S, dtype=torch.float32, device=dev)
    frame = torch.empty(S, dtype=torch.int32, device=dev)
    track = torch.empty(S, dtype=torch.int32, device=dev)
    src = torch.empty(S, dtype=torch.int32, device=dev)
    filled = torch.empty(S, dtype=torch.uint8, device=dev)
    # no workspace: the fused kernel keeps a tile and its halos in LDS (mega_refine_tracks_workspace_bytes is 0 at every
    # size; a library that wanted one would answer MEGA_ERR_WS here)
    _call("mega_refine_tracks", m_box, m_score, m_frame, m_off, o_off, K, M, S, int(bool(fill)), int(smooth),
          float(fill_scale), box, score, frame, track, src, filled, None, 0, prof=("refine_tracks",))
    return box, score, frame, track, src, filled


# ------------------------------------------------------------------------------------------------ tubelet AP
def tubelet_scores(score, off, use_max=False):
    """A tubelet's score as track_eval.py defines it (include/mega_hip.h mega_tubelet_scores).  score [M] f32: the members
    sorted by tubelet, then frame; off [U+1] i64.  -> [U] f64 on the device: the f64 sum in that order / the count, or the
    largest member with use_max."""
    M, U = score.shape[0], off.shape[0] - 1
    assert score.dtype == torch.float32 and off.dtype == torch.int64 and score.is_contiguous() and off.is_contiguous()
    assert score.shape == (M,) and off.shape == (U + 1,)
    out = torch.zeros(U, dtype=torch.float64, device=score.device)
    _call("mega_tubelet_scores", score, off, U, M, int(bool(use_max)), out, prof=("tubelet_scores",))
    return out


def tubelet_match(box, frame, rank, seg_off, ratio, gt_box, gt_track, gt_seg_off, tasks, offs, tubelet, tub_len, gt_len,
                  thresholds, F, C, n_pairs, ws_pairs, want_pairs=True, return_workspace=False):
    """Tubelets against GT tracks over T (video, label) tasks (include/mega_hip.h mega_tubelet_match).  box [M,4] f32,
    frame / rank [M] i32 sorted class-major then frame, seg_off [C*F+1] i64; ratio [F,2] f32; gt_box [Gb,4] f32, gt_track
    [Gb] i32 sorted the same way, gt_seg_off [C*F+1] i64; tasks [T,8] i32 (class, first frame, frames, p0, P, g0, G, 0),
    the most boxes first; offs [T,2] i64 (pair-table offset, workspace offset or -1); tubelet [slots] i32; tub_len [U]
    i32; gt_len [J] i32; thresholds: (num, den) pairs (host).  n_pairs: the sum of P * G; ws_pairs: that of the tasks whose
    table does not fit LDS.  -> match [R,U] u8 (0 outside the tasks), matched_gt [R,U] i32 (GT slot, -1: none), hits /
    both [n_pairs] i32 (None without want_pairs), on the device; with return_workspace also the workspace's two tables
    [ws_pairs] i32, preset to -1.  Does not synchronise."""
    M, Gb, T, U, J, slots = box.shape[0], gt_box.shape[0], tasks.shape[0], tub_len.shape[0], gt_len.shape[0], tubelet.shape[0]
    for t, dt in ((box, torch.float32), (frame, torch.int32), (rank, torch.int32), (seg_off, torch.int64),
                  (ratio, torch.float32), (gt_box, torch.float32), (gt_track, torch.int32), (gt_seg_off, torch.int64),
                  (tasks, torch.int32), (offs, torch.int64), (tubelet, torch.int32), (tub_len, torch.int32),
                  (gt_len, torch.int32)):
        assert t.dtype == dt and t.is_contiguous()
    assert box.shape == (M, 4) and frame.shape == (M,) and rank.shape == (M,) and seg_off.shape == (C * F + 1,)
    assert ratio.shape == (F, 2) and gt_box.shape == (Gb, 4) and gt_track.shape == (Gb,)
    assert gt_seg_off.shape == (C * F + 1,) and tasks.shape == (T, 8) and offs.shape == (T, 2)
    thr = [(int(n), int(d)) for n, d in thresholds]
    R = len(thr)
    thr_c = (ctypes.c_int * (2 * R))(*[v for nd in thr for v in nd])
    dev = box.device
    match = torch.zeros((R, U), dtype=torch.uint8, device=dev)
    matched_gt = torch.full((R, U), -1, dtype=torch.int32, device=dev)
    hits = torch.zeros(int(n_pairs), dtype=torch.int32, device=dev) if want_pairs else None
    both = torch.zeros(int(n_pairs), dtype=torch.int32, device=dev) if want_pairs else None
    nb = _lib.load().mega_tubelet_match_workspace_bytes(int(ws_pairs))
    ws = _ws(max(nb, 1), dev)
    if return_workspace:
        ws.fill_(0xFF)
    _call("mega_tubelet_match", box, frame, rank, seg_off, ratio, gt_box, gt_track, gt_seg_off, tasks, offs, tubelet,
          tub_len, gt_len, ctypes.cast(thr_c, ctypes.c_void_p), T, int(F), int(C), R, M, Gb, U, J, slots, int(n_pairs),
          int(ws_pairs), match, matched_gt, hits, both, ws, nb, prof=("tubelet_match",))
    if return_workspace:
        n, half = int(ws_pairs), nb // 2             # two arrays of n i32, each rounded up to 256 bytes
        tabs = (ws[:4 * n].view(torch.int32), ws[half:half + 4 * n].view(torch.int32))
        return match, matched_gt, hits, both, tabs
    return match, matched_gt, hits, both


# ------------------------------------------------------------------------------------------------ motion IoU
def motion_iou(gt_box, gt_track, gt_off, video_start, video_end, window, max_gt, return_workspace=False):
    """The motion IoU of every GT box (include/mega_hip.h mega_motion_iou; mega/pytorch_amd/motion_iou.py defines it).
    gt_box [G,4] f32, gt_track [G] i64, gt_off [F+1] i64, video_start / video_end [F] i32 (the frame range of each frame's
    video), window: W in 1..64, max_gt: the most boxes of one frame.  -> values [G] f64, counts [G] i32 on the device
    (counts preset to -1: a frame the kernel skipped keeps it); with return_workspace also the workspace's slots as
    [G, 2W] i32 (the pair IoUs' bits, -1: no neighbour; preset to -1), or None when no frame needs it.  Does not
    synchronise."""
    G, F, W = gt_box.shape[0], gt_off.shape[0] - 1, int(window)
    for t, dt in ((gt_box, torch.float32), (gt_track, torch.int64), (gt_off, torch.int64), (video_start, torch.int32),
                  (video_end, torch.int32)):
        assert t.dtype == dt and t.is_contiguous()
    assert gt_box.shape == (G, 4) and gt_track.shape == (G,) and gt_off.shape == (F + 1,)
    assert video_start.shape == (F,) and video_end.shape == (F,)
    dev = gt_box.device
    values = torch.zeros(G, dtype=torch.float64, device=dev)
    counts = torch.full((G,), -1, dtype=torch.int32, device=dev)
    nb = _lib.load().mega_motion_iou_workspace_bytes(G, W, int(max_gt))
    ws = _ws(max(nb, 1), dev)
    if return_workspace:
        ws.fill_(0xFF)
    _call("mega_motion_iou", gt_box, gt_track, gt_off, video_start, video_end, F, G, W, int(max_gt), values, counts, ws, nb,
          prof=("motion_iou",))
    if return_workspace:
        return values, counts, (ws[:8 * G * W].view(torch.int32).reshape(G, 2 * W) if nb else None)
    return values, counts


# ------------------------------------------------------------------------------------------------ error diagnosis
def diagnose_match(det_box, det_label, det_score, det_off, order, ratio, gt_box, gt_label, gt_off, C, max_gt, bg_thresh,
                   out=None):
    """The kind of every detection and the detections of every GT box (include/mega_hip.h mega_diagnose_match;
    mega/pytorch_amd/diagnose.py defines it).  det_box [N,4] f32, det_label [N] i32, det_score [N] f32, det_off [F+1] i64,
    order [N] i32 and ratio [F,2] f32 as for vid_eval_match, gt_box [G,4] f32, gt_label [G] i32, gt_off [F+1] i64.
    -> det_kind [N] u8, det_gt [N] i32, det_iou [N] f32, gt_det [3,G] i32 on the device, every element written by the
    kernel (out: such a tuple to write into instead of fresh tensors).  The kernel takes no workspace.  Does not
    synchronise."""
    N, F, G = det_box.shape[0], det_off.shape[0] - 1, gt_box.shape[0]
    for t, dt in ((det_box, torch.float32), (det_label, torch.int32), (det_score, torch.float32), (det_off, torch.int64),
                  (order, torch.int32), (ratio, torch.float32), (gt_box, torch.float32), (gt_label, torch.int32),
                  (gt_off, torch.int64)):
        assert t.dtype == dt and t.is_contiguous()
    assert det_box.shape == (N, 4) and det_label.shape == (N,) and det_score.shape == (N,) and order.shape == (N,)
    assert ratio.shape == (F, 2) and gt_box.shape == (G, 4) and gt_label.shape == (G,) and gt_off.shape == (F + 1,)
    dev = det_box.device
    if out is None:
        out = (torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
               torch.empty(N, dtype=torch.float32, device=dev), torch.empty((3, G), dtype=torch.int32, device=dev))
    det_kind, det_gt, det_iou, gt_det = out
    for t, dt, shape in ((det_kind, torch.uint8, (N,)), (det_gt, torch.int32, (N,)), (det_iou, torch.float32, (N,)),
                         (gt_det, torch.int32, (3, G))):
        assert t.dtype == dt and t.is_contiguous() and tuple(t.shape) == shape
    _call("mega_diagnose_match", det_box, det_label, det_score, det_off, order, ratio, gt_box, gt_label, gt_off, F, int(C),
          N, G, int(max_gt), float(bg_thresh), det_kind, det_gt, det_iou, gt_det, prof=("diagnose_match",))
    return det_kind, det_gt, det_iou, gt_det


# ------------------------------------------------------------------------------------------------ demo overlay
def overlay_detections(frames, boxes, scores, labels, counts, resized_hw, thr, thickness, palette, atlas,
                       select_only=False):
    """Draw the detections of F frames in place on the original-size frames (include/mega_hip.h mega_overlay_detections;
    mega/pytorch_amd/demo.py defines the picture).  frames [F,H,W,3] u8, boxes [F,R,4] f32 xyxy in the resized frame
    (resized_hw = its (height, width)), scores [F,R] f32, labels [F,R] i64 or i32, counts [F] i32, palette [NC,3] u8,
    atlas: demo.LabelAtlas.to(device) (cells [G,gh,gw] u8, advances [G] i32, class_glyphs [NC,ML] i32, fmt_glyphs [13] i32).
    Returns frames.  No synchronisation; nothing is copied to the host."""
    F, H, W = frames.shape[0], frames.shape[1], frames.shape[2]
    R = boxes.shape[1]
    assert frames.dtype == torch.uint8 and frames.shape == (F, H, W, 3) and frames.is_contiguous()
    assert boxes.dtype == torch.float32 and boxes.shape == (F, R, 4) and boxes.is_contiguous()
    assert scores.dtype == torch.float32 and scores.shape == (F, R) and scores.is_contiguous()
    assert labels.dtype in (torch.int64, torch.int32) and labels.shape == (F, R) and labels.is_contiguous()
    assert counts.dtype == torch.int32 and counts.shape == (F,) and counts.is_contiguous()
    assert palette.dtype == torch.uint8 and palette.dim() == 2 and palette.shape[1] == 3 and palette.is_contiguous()
    NC = palette.shape[0]
    G, gh, gw = atlas.cells.shape
    assert atlas.cells.dtype == torch.uint8 and atlas.cells.is_contiguous()
    assert atlas.advances.dtype == torch.int32 and atlas.advances.shape == (G,)
    assert atlas.class_glyphs.dtype == torch.int32 and atlas.class_glyphs.shape[0] == NC and atlas.class_glyphs.is_contiguous()
    assert atlas.fmt_glyphs.dtype == torch.int32 and atlas.fmt_glyphs.shape == (13,)
    ML = atlas.class_glyphs.shape[1]
    rh, rw = int(resized_hw[0]), int(resized_hw[1])
    # BoxList.resize: the ratio is a Python float (f64 division), the multiply an f32 tensor op with the ratio rounded to f32
    sx, sy = float(torch.tensor(W / rw, dtype=torch.float32)), float(torch.tensor(H / rh, dtype=torch.float32))
    nb = _lib.load().mega_overlay_detections_workspace_bytes(F, R)
    ws = _ws(max(nb, 1), frames.device)
    _call("mega_overlay_detections", frames, F, H, W, boxes, scores, labels, int(labels.dtype == torch.int64), counts, R,
          sx, sy, float(thr), int(thickness), palette, NC, atlas.class_glyphs, ML, atlas.fmt_glyphs, atlas.cells,
          atlas.advances, G, gh, gw, int(bool(select_only)), ws, nb, prof=("overlay",))
    return frames


# ------------------------------------------------------------------------------------------------ JPEG decode
def _host_u8(data):
    """a bytes-like object in host memory as a uint8 numpy view (no copy): its .ctypes.data is what the C ABI reads"""
    import numpy as np
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    assert a.dtype == np.uint8 and a.ndim == 1 and a.flags.c_contiguous
    return a


def jpeg_probe(data):
    """include/mega_hip.h mega_jpeg_probe on the JPEG bytes `data` (host): the int32 info array [12] (jpeg.Info reads it).
    Raises jpeg.Unsupported for a stream outside the accepted set.  Host only: no device, no stream."""
    import numpy as np
    from . import jpeg
    a = _host_u8(data)
    info = np.zeros(jpeg.INFO_INTS, dtype=np.int32)
    if _lib.load().mega_jpeg_probe(a.ctypes.data, a.size, info.ctypes.data) != 0:
        raise jpeg.Unsupported("not a JPEG this decoder accepts (mega/pytorch_amd/jpeg.py lists the accepted streams)")
    return info


def jpeg_entropy_decode(data, info, out=None):
    """include/mega_hip.h mega_jpeg_entropy_decode: the quantisation tables and raw int16 DCT coefficients of the JPEG bytes
    `data` into `out` (a writable, contiguous int16 numpy array of at least info.coef_elems elements -- a slot of a pinned
    staging buffer, say) or a new array.  info: the jpeg.Info the stream must agree with in size, components and sampling.
    ctypes releases the GIL around the call.  Raises jpeg.Unsupported (refused, or other frames than info's) or jpeg.Corrupt."""
    import numpy as np
    from . import jpeg
    a = _host_u8(data)
    if out is None:
        out = np.empty(info.coef_elems, dtype=np.int16)
    assert out.dtype == np.int16 and out.ndim == 1 and out.flags.c_contiguous and out.flags.writeable
    assert out.size >= info.coef_elems
    lib = _lib.load()
    if lib.mega_jpeg_entropy_decode(a.ctypes.data, a.size, info.array.ctypes.data, out.ctypes.data, out.size) != 0:
        got = np.zeros(jpeg.INFO_INTS, dtype=np.int32)
        if lib.mega_jpeg_probe(a.ctypes.data, a.size, got.ctypes.data) != 0:
            raise jpeg.Unsupported("not a JPEG this decoder accepts")
        if not jpeg.Info(got).same_frames(info):
            raise jpeg.Unsupported("the stream is %s, expected %s" % (tuple(got[:4]), tuple(info.array[:4])))
        raise jpeg.Corrupt("truncated or corrupt entropy-coded data")
    return out


def jpeg_reconstruct(coef, info, out=None):
    """include/mega_hip.h mega_jpeg_reconstruct: coef int16 [N, stride] on the device, every row one frame in the layout of
    jpeg_entropy_decode (stride % 8 == 0, >= info.coef_elems) -> uint8 RGB [N, H, W, 3].  out: optional contiguous tensor of
    that shape to write into."""
    assert coef.dtype == torch.int16 and coef.dim() == 2 and coef.is_contiguous()
    N, stride = coef.shape
    H, W = info.hw
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=coef.device)
    else:
        assert out.shape == (N, H, W, 3) and out.dtype == torch.uint8 and out.is_contiguous()
    nb = _lib.load().mega_jpeg_reconstruct_workspace_bytes(N, H, W, info.sampling)
    # the component planes: taken like the output, with torch.empty (tests/test_jpeg_gpu.py poisons both through its proxy)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=coef.device)
    _call("mega_jpeg_reconstruct", coef, stride, N, H, W, info.sampling, out, ws, nb,
          prof=("jpeg", 0.0, coef.numel() * 2.0 + out.numel() + 2.0 * nb))
    return out
