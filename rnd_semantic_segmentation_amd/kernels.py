"""Tensor-level wrappers over the C-ABI (torch is plumbing: device memory + streams).

Layout: every activation handled here is an NHWC-contiguous tensor [B,H,W,C]
(bf16 unless stated).  Callers that hold NCHW-shaped channels_last tensors pass
`x.permute(0, 2, 3, 1)` (a free view).
"""
import collections
import ctypes
import math

import torch

from . import _lib
from ._lib import check

EPI_SCALE_BIAS, EPI_RESIDUAL, EPI_RELU, EPI_MASK, EPI_OUT_F32, EPI_ZSPLIT, EPI_WRITE_MASK, EPI_BITMASK, EPI_LEAKY = 1, 2, 4, 8, 16, 32, 64, 128, 256
GATHER_FWD, GATHER_DGRAD = 0, 1
ASPP_ZGW, ASPP_KPAD = 20, 704


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-launch timing with HIP events on the launch stream (bench.py): set to a list to collect
# (kernel_name, start_event, stop_event, algorithmic_flops) tuples; None = no overhead.
PROFILE = None


def _timed(name, flops, launch, tag=None):
    if PROFILE is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = launch()
    e1.record()
    PROFILE.append((name, e0, e1, flops, tag))
    return rc


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _chk(t, dtype, name):
    if not t.is_cuda:
        raise _lib.MiError("%s must live on the GPU (no CPU path exists)" % name)
    if t.dtype != dtype:
        raise _lib.MiError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.MiError("%s must be contiguous" % name)
    return t


# Optional record of what the conv launches of this module ran (the protocol of gk.ROUTES): set to a set() to collect the ConvPlan / WgradPlan of every
# conv_gemm, conv_gemm_stats and conv_wgrad call (the host queries below, which share their planning functions with the launches); None = no overhead.
ROUTES = None


class ConvPlan(collections.namedtuple("ConvPlan", "flags kernel mt unit pref staged epi korder m_tiles n_tiles rounds slots")):
    """flags (the epilogue flags of the call), then include/mi355seg.h mi_conv_gemm_plan's descriptor (MI_CPLAN_LEN fields, in its order).  `name` separates
    every instantiation the product library launches; a generic epilogue (epi -1) is named by the flags it reads, g<flags>."""
    __slots__ = ()

    @property
    def name(self):
        epi = "stats" if self.epi == 512 else ("e%d" % self.epi if self.epi >= 0 else "g%d" % self.flags)
        if self.kernel == 1:
            return "pp.mtg%d.%s.k%d" % (self.mt, epi, self.korder)
        return "nt.mt%d.%s%s.%s%s" % (self.mt, "unit" if self.unit else "gen", ".pref" if self.pref else "", epi, ".stg" if self.staged else "")


class WgradPlan(collections.namedtuple("WgradPlan", "out_map kernel mode S steps step_rows o_tiles i_tiles deferred")):
    """out_map of the call, then include/mi355seg.h mi_conv_wgrad_plan's descriptor (MI_WPLAN_LEN fields, in its order).  `name`: main kernel (with its
    addressing mode), .aspp for the scattering reducer of out_map 1, .deferred for the mi_conv_wgrad_partial form."""
    __slots__ = ()

    @property
    def name(self):
        k = ("tn.m%d" % self.mode, "tn256.m%d" % self.mode, "p3", "q3", "s4")[self.kernel]
        return k + (".aspp" if self.out_map else "") + (".deferred" if self.deferred else "")


CPLAN_LEN, WPLAN_LEN = len(ConvPlan._fields) - 1, len(WgradPlan._fields) - 1        # MI_CPLAN_LEN, MI_WPLAN_LEN (tests/test_host_conv_routes.py)


def conv_gemm_plan(a_shape, N, out_hw, ksize=1, stride=1, pad=0, dil=1, flags=0, wide=None):
    """What conv_gemm (wide: its `wide`) / conv_gemm_stats (flags 512) launch for an a of shape [B,Ha,Wa,Ca]: host only.  wide: None, 0, 8 or 10 - the
    query knows the product library's tile heights only, so while ROUTES records, conv_gemm(wide=108 | 110) (the rolling loop of experiment builds) and
    arguments no plan exists for raise here, before the launch that would have refused them."""
    B, Ha, Wa, Ca = a_shape
    r = (ctypes.c_int * CPLAN_LEN)()
    check(_lib.lib().mi_conv_gemm_plan(B, Ha, Wa, Ca, out_hw[0], out_hw[1], N, ksize, stride, pad, dil, flags, -1 if wide is None else int(wide), r),
          "mi_conv_gemm_plan")
    return ConvPlan(flags, *r)


def conv_wgrad_plan(dy_shape, x_shape, ksize=1, stride=1, pad=0, dil=1, out_map=0, deferred=False):
    """What conv_wgrad (deferred: its batch= form) launches for dy [B,Ho,Wo,O] and x [B,Ha,Wa,I]: host only."""
    B, Ho, Wo, O = dy_shape
    _, Ha, Wa, I = x_shape
    r = (ctypes.c_int * WPLAN_LEN)()
    check(_lib.lib().mi_conv_wgrad_plan(B, Ha, Wa, I, Ho, Wo, O, ksize, stride, pad, dil, out_map, int(deferred), r), "mi_conv_wgrad_plan")
    return WgradPlan(out_map, *r)


def pack_weight_fwd(w, out=None):
    """fp32 OIHW -> bf16 [k*k][O][I]"""
    _chk(w, torch.float32, "w")
    O, I, k, _ = w.shape
    if out is None:
        out = torch.empty((k * k, O, I), dtype=torch.bfloat16, device=w.device)
    check(_lib.lib().mi_pack_weight_fwd(_p(w), _p(out), O, I, k, _stream()), "mi_pack_weight_fwd")
    return out


def pack_weight_dgrad(w, scale=None, out=None):
    """fp32 OIHW -> bf16 [k*k][I][O], FrozenBN scale[o] folded in"""
    _chk(w, torch.float32, "w")
    O, I, k, _ = w.shape
    if out is None:
        out = torch.empty((k * k, I, O), dtype=torch.bfloat16, device=w.device)
    check(_lib.lib().mi_pack_weight_dgrad(_p(w), _p(scale), _p(out), O, I, k, _stream()), "mi_pack_weight_dgrad")
    return out


def pack_weights_multi(wflat, sflat, wp, wpt, table_dev, n_desc, total_blocks):
    """One launch packing every conv weight described by `table_dev` (see include/mi355seg.h)."""
    check(_lib.lib().mi_pack_weights_multi(_p(wflat), _p(sflat), _p(wp), _p(wpt), _p(table_dev), n_desc, total_blocks, _stream()),
          "mi_pack_weights_multi")


def conv_gemm(a, wp, out_hw, ksize=1, stride=1, pad=0, dil=1, mode=GATHER_FWD, scale=None, bias=None, res=None,
              msk=None, relu=False, out_f32=False, zsplit=0, out=None, bits=None, mask_out=None, leaky=0.0, flop_cols=0, wide=None):
    """out[b,ho,wo,n] = epi(sum_{t,c} a[b,src(ho,wo,t),c] * wp[t,n,c]);  a [B,Ha,Wa,Ca] bf16, wp [k*k,N,Ca] bf16.
    msk: bf16 [B,Ho,Wo,N] ReLU mask source; bits: the same mask as packed sign bits (int16 [B,Ho,Wo,N/16]);
    mask_out: int16 [B,Ho,Wo,N/16] receiving the sign bits of the result.
    flop_cols: live columns of a padded ASPP operand (per zsplit plane, or of Ca == 704), for the FLOP accounting only.
    wide: None = the library's own choice of main loop; 8 / 10 = force the wide-tile ping-pong loop (mi_conv_gemm_pp) with that
    many 16-row MFMA tiles per wave (tests, tools/ppexp.py)."""
    _chk(a, torch.bfloat16, "a")
    _chk(wp, torch.bfloat16, "wp")
    B, Ha, Wa, Ca = a.shape
    T, N, Cw = wp.shape
    if T != ksize * ksize or Cw != Ca:
        raise _lib.MiError("packed weight %s does not match ksize=%d, Ca=%d" % (tuple(wp.shape), ksize, Ca))
    Ho, Wo = out_hw
    flags = 0
    if scale is not None:
        flags |= EPI_SCALE_BIAS
        _chk(scale, torch.float32, "scale")
        _chk(bias, torch.float32, "bias")
    if res is not None:
        flags |= EPI_RESIDUAL
        _chk(res, torch.bfloat16, "res")
        assert tuple(res.shape) == (B, Ho, Wo, N)
    if relu:
        flags |= EPI_RELU
    if leaky:
        flags |= EPI_LEAKY          # LeakyReLU(leaky) forward (with relu=True) or its backward (with bits=...)
    if msk is not None:
        flags |= EPI_MASK
        _chk(msk, torch.bfloat16, "msk")
        assert tuple(msk.shape) == (B, Ho, Wo, N)
    if bits is not None:
        flags |= EPI_BITMASK
        _chk(bits, torch.int16, "bits")
        assert tuple(bits.shape) == (B, Ho, Wo, N // 16) and msk is None
        msk = bits
    if mask_out is not None:
        flags |= EPI_WRITE_MASK
        _chk(mask_out, torch.int16, "mask_out")
        assert tuple(mask_out.shape) == (B, Ho, Wo, N // 16)
    if zsplit:
        flags |= EPI_ZSPLIT | EPI_OUT_F32
        if out is None:
            out = torch.empty((N // zsplit, B * Ho * Wo, zsplit), dtype=torch.float32, device=a.device)
    elif out_f32:
        flags |= EPI_OUT_F32
        if out is None:
            out = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=a.device)
    elif out is None:
        out = torch.empty((B, Ho, Wo, N), dtype=torch.bfloat16, device=a.device)
    _chk(out, torch.float32 if (zsplit or out_f32) else torch.bfloat16, "out")
    if out.numel() != B * Ho * Wo * N:
        raise _lib.MiError("out has %d elements, the conv writes %d" % (out.numel(), B * Ho * Wo * N))
    # algorithmic FLOPs (2 * pixels * C_out * C_in * k^2), padding columns of the ASPP operands excluded
    n_real = N * flop_cols // zsplit if (zsplit and flop_cols) else N
    ca_real = flop_cols if (Ca == ASPP_KPAD and flop_cols) else Ca
    flops = 2.0 * B * Ho * Wo * n_real * ca_real * ksize * ksize
    if ROUTES is not None:
        ROUTES.add(conv_gemm_plan(a.shape, N, out_hw, ksize, stride, pad, dil, flags, wide))
    if wide is not None:
        check(_lib.lib().mi_conv_gemm_pp(_p(a), _p(wp), _p(out), B, Ha, Wa, Ca, Ho, Wo, N, ksize, stride, pad, dil, mode, _p(scale), _p(bias), _p(res),
                                         _p(msk), _p(mask_out), flags, zsplit, float(leaky), int(wide), _stream()), "mi_conv_gemm_pp")
        return out
    kern = "igemm_nt_kernel"
    if PROFILE is not None and _lib.lib().mi_conv_gemm_route(B, Ha, Wa, Ca, Ho, Wo, N, ksize, stride, flags):
        kern = "igemm_pp_kernel"
    check(_timed(kern, flops, lambda: _lib.lib().mi_conv_gemm(
        _p(a), _p(wp), _p(out), B, Ha, Wa, Ca, Ho, Wo, N, ksize, stride, pad, dil, mode,
        _p(scale), _p(bias), _p(res), _p(msk), _p(mask_out), flags, zsplit, float(leaky), _stream()),
        tag=("dgrad" if mode == GATHER_DGRAD else "fwd", ksize, Ca, N, B * Ho * Wo, flags, dil)), "mi_conv_gemm")
    return out


_ws_cache = {}


def conv_gemm_stats(a, wp, out_hw, ksize, stride, pad, dil, pilot, bn=None, out=None, sums=None):
    """conv_gemm with a plain bf16 store that also returns the BatchNorm statistics of its output, taken in the epilogue: (out, sums, fin) with
    sums[0][n] = sum (out - pilot[n]), sums[1][n] = sum (out - pilot[n])^2 ([2, N] fp32) - bn_colsum2(out, pilot) without the extra read.
    bn (an nn.BatchNorm2d whose statistics are NOT shared across ranks): the last reduction launch also finalizes them (bn_finalize's result `fin`
    and running-statistics update, count = the pixels of this tensor); otherwise fin is None.  out / sums: tensors to write into (tests: carved from
    sentinel-filled allocations)."""
    _chk(a, torch.bfloat16, "a")
    _chk(wp, torch.bfloat16, "wp")
    _chk(pilot, torch.float32, "pilot")
    B, Ha, Wa, Ca = a.shape
    T, N, Cw = wp.shape
    if T != ksize * ksize or Cw != Ca:
        raise _lib.MiError("packed weight %s does not match ksize=%d, Ca=%d" % (tuple(wp.shape), ksize, Ca))
    Ho, Wo = out_hw
    if out is None:
        out = torch.empty((B, Ho, Wo, N), dtype=torch.bfloat16, device=a.device)
    if sums is None:
        sums = torch.empty((2, N), dtype=torch.float32, device=a.device)
    _chk(out, torch.bfloat16, "out")
    _chk(sums, torch.float32, "sums")
    if out.numel() != B * Ho * Wo * N or sums.numel() != 2 * N:
        raise _lib.MiError("out / sums have %d / %d elements, the conv writes %d / %d" % (out.numel(), sums.numel(), B * Ho * Wo * N, 2 * N))
    ws = _workspace(int(_lib.lib().mi_conv_gemm_stats_workspace(B * Ho * Wo, N)), a.device, "conv_stats")
    fin, fa = None, (None, None, None, None, None, 0.0, 0.0, None)
    if bn is not None:
        track = bn.track_running_stats and bn.running_mean is not None
        if track and bn.momentum is None:
            raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not used by the reference")
        fin = torch.empty((4, N), dtype=torch.float32, device=a.device)
        fa = (_p(bn.weight.detach()), _p(bn.bias.detach()), _p(bn.running_mean) if track else None, _p(bn.running_var) if track else None,
              _p(bn.num_batches_tracked) if track else None, float(bn.momentum or 0.0), float(bn.eps), _p(fin))
    flops = 2.0 * B * Ho * Wo * N * Ca * ksize * ksize
    if ROUTES is not None:
        ROUTES.add(conv_gemm_plan(a.shape, N, out_hw, ksize, stride, pad, dil, 512))
    _timed("igemm_stats", flops, lambda: check(_lib.lib().mi_conv_gemm_stats(_p(a), _p(wp), _p(out), B, Ha, Wa, Ca, Ho, Wo, N, ksize, stride, pad, dil, _p(pilot),
                                                                             _p(sums), _p(ws), ws.numel(), *fa, _stream()), "mi_conv_gemm_stats"),
           ("fwd", ksize, Ca, N, B * Ho * Wo, 512, dil))
    return out, sums, fin


def _workspace(nbytes, device, tag="ws"):
    # one buffer per (purpose, device, stream): launches on one stream are ordered, so they can share it; two streams cannot
    key = (tag, str(device), torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def conv_chain(a, w_first, res, w_second, scale1=None, shift1=None, scale2=None, shift2=None, bits1=None, bits2=None, mid=None, out=None,
               bits1_out=None, bits2_out=None, grid=0):
    """Two chained 1x1 convs in one launch (csrc/chain.hip).  Forward (scale1 given): mid = relu(scale1 * a.w_first^T + shift1 + res),
    out = relu(scale2 * mid.w_second^T + shift2), returns (mid, out, bits(mid), bits(out)).  Backward (bits1 given): mid = (a.w_first^T + res) masked by
    bits1, out = (mid.w_second^T) masked by bits2, returns (mid, out).  a [B,H,W,K1], res [B,H,W,N1] bf16 NHWC; w_first [1,N1,K1], w_second [1,N2,N1]."""
    _chk(a, torch.bfloat16, "a")
    _chk(res, torch.bfloat16, "res")
    _chk(w_first, torch.bfloat16, "w_first")
    _chk(w_second, torch.bfloat16, "w_second")
    B, H, W, K1 = a.shape
    N1, N2 = w_first.shape[-2], w_second.shape[-2]
    if w_first.shape[-1] != K1 or w_second.shape[-1] != N1 or tuple(res.shape) != (B, H, W, N1):
        raise _lib.MiError("conv_chain: a %s, w_first %s, res %s, w_second %s do not chain" % (tuple(a.shape), tuple(w_first.shape), tuple(res.shape), tuple(w_second.shape)))
    backward = bits1 is not None
    M = B * H * W
    if mid is None:
        mid = torch.empty((B, H, W, N1), dtype=torch.bfloat16, device=a.device)
    if out is None:
        out = torch.empty((B, H, W, N2), dtype=torch.bfloat16, device=a.device)
    _chk(mid, torch.bfloat16, "mid")
    _chk(out, torch.bfloat16, "out")
    if mid.numel() != M * N1 or out.numel() != M * N2:
        raise _lib.MiError("conv_chain: mid / out have the wrong size")
    if backward:
        _chk(bits1, torch.int16, "bits1")
        _chk(bits2, torch.int16, "bits2")
        assert bits1.numel() == M * N1 // 16 and bits2.numel() == M * N2 // 16
    else:
        for t, n in ((scale1, N1), (shift1, N1), (scale2, N2), (shift2, N2)):
            _chk(t, torch.float32, "scale / shift")
            assert t.numel() == n
        if bits1_out is None:
            bits1_out = torch.empty((B, H, W, N1 // 16), dtype=torch.int16, device=a.device)
        if bits2_out is None:
            bits2_out = torch.empty((B, H, W, N2 // 16), dtype=torch.int16, device=a.device)
        _chk(bits1_out, torch.int16, "bits1_out")
        _chk(bits2_out, torch.int16, "bits2_out")
        assert bits1_out.numel() == M * N1 // 16 and bits2_out.numel() == M * N2 // 16
    flops = 2.0 * M * N1 * (K1 + N2)
    check(_timed("chain_kernel", flops, lambda: _lib.lib().mi_conv_chain(
        _p(a), _p(w_first), _p(res), _p(mid), _p(w_second), _p(out), M, K1, N1, N2, _p(scale1), _p(shift1), _p(scale2), _p(shift2),
        _p(bits1), _p(bits2), _p(bits1_out), _p(bits2_out), 1 if backward else 0, int(grid), _stream()),
        tag=("chain_bwd" if backward else "chain_fwd", 1, K1, N1, M, 0, 1)), "mi_conv_chain")
    return (mid, out) if backward else (mid, out, bits1_out, bits2_out)


class WgradBatch:
    """The slab reducers of up to eight weight gradients as ONE launch (mi_conv_wgrad_partial + mi_conv_wgrad_reduce): conv_wgrad(..., batch=b) runs the
    main kernel only and keeps its split-K slabs in a workspace of its own; b.flush() (same stream, after the last of them) sums them all.  Same bits as
    the one-call form, except where the fused-row 3x3 split applies: mi_conv_wgrad_partial plans it for 448 workgroup slots (a launch beside a
    data-gradient chain), mi_conv_wgrad for 512, so the fp32 partial sums are partitioned differently.  A full batch flushes itself."""
    MAX = 8

    def __init__(self):
        self._n = 0
        self._size = int(_lib.lib().mi_conv_wgrad_job_bytes())
        self._jobs = ctypes.create_string_buffer(self.MAX * self._size)
        self._keep = []

    def slot(self):
        if self._n == self.MAX:
            self.flush()
        return self._n, ctypes.c_void_p(ctypes.addressof(self._jobs) + self._n * self._size)

    def added(self, *tensors):
        self._n += 1
        self._keep.extend(tensors)

    def flush(self):
        if self._n:
            check(_timed("wgrad_reduce_multi_kernel", 0.0, lambda: _lib.lib().mi_conv_wgrad_reduce(self._jobs, self._n, _stream()), tag=("wgrad_reduce", 1, 0, 0, 0, 0, 1)),
                  "mi_conv_wgrad_reduce")
            self._n, self._keep = 0, []


def conv_wgrad(dy, x, dw, ksize=1, stride=1, pad=0, dil=1, scale=None, accumulate=False, out_map=0, ncls=0, batch=None):
    """dw[o,i,ky,kx] (+)= scale[o] * sum_m dy[m,o] x[src(m,t),i];  dy [B,Ho,Wo,O], x [B,Ha,Wa,I] bf16; dw fp32.
    out_map=1 (ASPP): dy is the im2col matrix with 36*ncls live columns, dw the 4 stacked [ncls,I,3,3] gradients.
    batch (a WgradBatch): the slab reducer is deferred to batch.flush()."""
    _chk(dy, torch.bfloat16, "dy")
    _chk(x, torch.bfloat16, "x")
    _chk(dw, torch.float32, "dw")
    B, Ho, Wo, O = dy.shape
    _, Ha, Wa, I = x.shape
    L = _lib.lib()
    need = L.mi_conv_wgrad_workspace(B, Ho, Wo, O, I, ksize)
    if out_map == 1 and not 0 < 36 * ncls <= O:
        raise _lib.MiError("conv_wgrad(out_map=1) needs ncls with 36*ncls <= %d, got %r" % (O, ncls))
    o_real = 36 * ncls if out_map == 1 else O
    flops = 2.0 * B * Ho * Wo * o_real * I * ksize * ksize
    kern = "wgrad_tn_kernel+reduce"
    if PROFILE is not None:
        kern = ("wgrad_tn_kernel", "wgrad_tn256_kernel", "wgrad_p3_kernel", "wgrad_q3_kernel", "wgrad_s4_kernel")[
            L.mi_conv_wgrad_route(B, Ha, Wa, I, Ho, Wo, O, ksize, stride, pad, dil, out_map)] + "+reduce"
    if ROUTES is not None:
        ROUTES.add(conv_wgrad_plan(dy.shape, x.shape, ksize, stride, pad, dil, out_map, batch is not None))
    if batch is not None:
        idx, job = batch.slot()
        ws = _workspace(need, dy.device, "wgrad_b%d" % idx)             # its slabs must survive until the flush: one buffer per batch slot and stream
        check(_timed(kern.replace("+reduce", ""), flops, lambda: L.mi_conv_wgrad_partial(
            _p(dy), _p(x), _p(dw), B, Ha, Wa, I, Ho, Wo, O, ksize, stride, pad, dil, _p(scale),
            int(accumulate), out_map, int(ncls), dw.numel(), _p(ws), ws.numel(), job, _stream()), tag=("wgrad", ksize, I, O, B * Ho * Wo, out_map, dil)), "mi_conv_wgrad_partial")
        batch.added(ws, dw, scale)
        return dw
    ws = _workspace(need, dy.device, "wgrad")
    check(_timed(kern, flops, lambda: L.mi_conv_wgrad(
        _p(dy), _p(x), _p(dw), B, Ha, Wa, I, Ho, Wo, O, ksize, stride, pad, dil, _p(scale),
        int(accumulate), out_map, int(ncls), dw.numel(), _p(ws), ws.numel(), _stream()), tag=("wgrad", ksize, I, O, B * Ho * Wo, out_map, dil)), "mi_conv_wgrad")
    return dw


def _rates(rates):
    return (ctypes.c_int * 4)(*[int(r) for r in rates])


def aspp_pack_fwd(w4, out=None):
    """[4,K,C,3,3] fp32 -> Wall bf16 [1, 720, C] (packed-weight form for conv_gemm, ksize 1)"""
    _chk(w4, torch.float32, "w4")
    R, K, C = w4.shape[:3]
    if out is None:
        out = torch.empty((1, 36 * ASPP_ZGW, C), dtype=torch.bfloat16, device=w4.device)
    check(_lib.lib().mi_aspp_pack_fwd(_p(w4), _p(out), C, K, _stream()), "mi_aspp_pack_fwd")
    return out


def aspp_pack_dgrad(w4, out=None):
    """[4,K,C,3,3] fp32 -> WallT bf16 [1, C, 704]"""
    _chk(w4, torch.float32, "w4")
    R, K, C = w4.shape[:3]
    if out is None:
        out = torch.empty((1, C, ASPP_KPAD), dtype=torch.bfloat16, device=w4.device)
    check(_lib.lib().mi_aspp_pack_dgrad(_p(w4), _p(out), C, K, _stream()), "mi_aspp_pack_dgrad")
    return out


def aspp_col2im(z, bias4, B, H, W, K, rates):
    _chk(z, torch.float32, "z")
    _chk(bias4, torch.float32, "bias4")
    low = torch.empty((B, H, W, K), dtype=torch.float32, device=z.device)
    check(_timed("aspp_col2im_kernel", 0.0, lambda: _lib.lib().mi_aspp_col2im(_p(z), _p(bias4), _p(low), B, H, W, K, _rates(rates), _stream()),
                 tag=("aspp_aux", 0, 0, 0, B * H * W, 0, 0)), "mi_aspp_col2im")
    return low


def aspp_im2col(dlow, rates):
    _chk(dlow, torch.float32, "dlow")
    B, H, W, K = dlow.shape
    g = torch.empty((B, H, W, ASPP_KPAD), dtype=torch.bfloat16, device=dlow.device)
    check(_timed("aspp_im2col_kernel", 0.0, lambda: _lib.lib().mi_aspp_im2col(_p(dlow), _p(g), B, H, W, K, _rates(rates), _stream()),
                 tag=("aspp_aux", 0, 0, 0, B * H * W, 0, 0)), "mi_aspp_im2col")
    return g


def aspp_bias_grad(dlow, dbias4, accumulate=False):
    _chk(dlow, torch.float32, "dlow")
    _chk(dbias4, torch.float32, "dbias4")
    B, H, W, K = dlow.shape
    L = _lib.lib()
    ws = _workspace(L.mi_colsum_workspace(B * H * W, K), dlow.device, "colsum")
    check(_timed("colsum_kernels", 0.0, lambda: L.mi_aspp_bias_grad(_p(dlow), _p(dbias4), B * H * W, K, int(accumulate), _p(ws), ws.numel(), _stream()),
                 tag=("aspp_aux", 0, 0, 0, B * H * W, 0, 0)), "mi_aspp_bias_grad")
    return dbias4


def upsample_ac_fwd(low, size):
    """low [B,h,w,K] fp32 NHWC -> up [B,K,H,W] fp32 NCHW"""
    _chk(low, torch.float32, "low")
    B, h, w, K = low.shape
    H, W = size
    up = torch.empty((B, K, H, W), dtype=torch.float32, device=low.device)
    check(_lib.lib().mi_upsample_ac_fwd(_p(low), _p(up), B, h, w, K, H, W, _stream()), "mi_upsample_ac_fwd")
    return up


def upsample_ac_bwd(dup, low_hw):
    _chk(dup, torch.float32, "dup")
    B, K, H, W = dup.shape
    h, w = low_hw
    dlow = torch.empty((B, h, w, K), dtype=torch.float32, device=dup.device)
    check(_lib.lib().mi_upsample_ac_bwd(_p(dup), _p(dlow), B, h, w, K, H, W, _stream()), "mi_upsample_ac_bwd")
    return dlow


def softmax_ce_fwd(logits, labels, ignore_index=255):
    """logits [B,K,H,W] fp32, labels [B,H,W] int64 -> loss_out fp32[4] = (mean loss, n_valid, out-of-range labels, scratch)"""
    _chk(logits, torch.float32, "logits")
    _chk(labels, torch.int64, "labels")
    B, K, H, W = logits.shape
    L = _lib.lib()
    ws = _workspace(L.mi_ce_workspace(B, H, W), logits.device, "ce")
    out = torch.empty(4, dtype=torch.float32, device=logits.device)
    check(L.mi_softmax_ce_fwd(_p(logits), _p(labels), _p(out), B, K, H, W, ignore_index, _p(ws), ws.numel(), _stream()),
          "mi_softmax_ce_fwd")
    return out


def softmax_ce_bwd(logits, labels, loss_out, grad_scale=1.0, ignore_index=255):
    _chk(logits, torch.float32, "logits")
    _chk(labels, torch.int64, "labels")
    B, K, H, W = logits.shape
    d = torch.empty_like(logits)
    check(_lib.lib().mi_softmax_ce_bwd(_p(logits), _p(labels), _p(loss_out), _p(d), B, K, H, W, ignore_index,
                                        float(grad_scale), _stream()), "mi_softmax_ce_bwd")
    return d


def _head_buffers(low, target, workspace, tag, want_grad, target_dtype=torch.int64, target_name="labels"):
    """What the fused upsample + loss wrappers share: low [B,h,w(,K)] fp32 and target [B,H,W] checked -> (dims = B, h, w(, K), H, W: the size
    arguments of `workspace` and of the launch; the workspace; loss_out[4]; dlow or None)."""
    _chk(low, torch.float32, "low")
    _chk(target, target_dtype, target_name)
    dims = tuple(low.shape) + tuple(target.shape[1:])
    ws = _workspace(workspace(*dims), low.device, tag)
    return dims, ws, torch.empty(4, dtype=torch.float32, device=low.device), (torch.empty_like(low) if want_grad else None)


def _chk_class_weights(class_weights, low, who):
    """class_weights: None, or one fp32 weight per class of low [B,h,w,K] on low's device."""
    if class_weights is not None:
        _chk(class_weights, torch.float32, "class_weights")
        K = low.shape[-1]
        if tuple(class_weights.shape) != (K,) or class_weights.device != low.device:
            raise _lib.MiError("%s: class_weights must be [%d] on %s, got %s on %s" % (who, K, low.device, tuple(class_weights.shape), class_weights.device))


def upsample_ce(low, labels, want_grad=True, grad_scale=1.0, ignore_index=255, align_corners=True, class_weights=None, label_smoothing=0.0):
    """Fused classifier-upsample + CrossEntropyLoss.  Returns (loss_out[4], dlow or None).  align_corners False: F.interpolate(size=) default.
    class_weights ([K] fp32 on low's device) / label_smoothing: CrossEntropyLoss(weight=, label_smoothing=) through mi_upsample_ce_w, where
    loss_out[1] is the weight sum of the valid pixels; with both at their defaults the call is mi_upsample_ce_ex as ever."""
    L = _lib.lib()
    dims, ws, out, dlow = _head_buffers(low, labels, L.mi_upsample_ce_workspace, "upce", want_grad)
    if class_weights is None and float(label_smoothing) == 0.0:
        check(L.mi_upsample_ce_ex(_p(low), _p(labels), _p(out), _p(dlow), *dims, ignore_index, float(grad_scale), int(bool(align_corners)),
                                  _p(ws), ws.numel(), _stream()), "mi_upsample_ce")
        return out, dlow
    _chk_class_weights(class_weights, low, "upsample_ce")
    check(L.mi_upsample_ce_w(_p(low), _p(labels), _p(class_weights), _p(out), _p(dlow), *dims, ignore_index, float(label_smoothing),
                             float(grad_scale), int(bool(align_corners)), _p(ws), ws.numel(), _stream()), "mi_upsample_ce_w")
    return out, dlow


def check_ohem(ohem):
    """(thresh, min_kept) of an OHEM criterion, checked: 0 <= thresh <= 1, min_kept an integer >= 1."""
    try:
        thresh, min_kept = ohem
        thresh, mk = float(thresh), int(min_kept)
    except (TypeError, ValueError):
        raise ValueError("ohem must be (thresh, min_kept), got %r" % (ohem,))
    if not 0.0 <= thresh <= 1.0:
        raise ValueError("ohem: thresh %r lies outside [0, 1]" % (thresh,))
    if mk < 1 or mk != min_kept:
        raise ValueError("ohem: min_kept must be an integer >= 1, got %r" % (min_kept,))
    return thresh, mk


def refuse_ohem_with_weights(ohem, class_weights, label_smoothing):
    """OHEM together with CrossEntropyLoss's weight= / label_smoothing= is not built yet: every layer refuses the pair with this message."""
    if ohem is not None and (class_weights is not None or float(label_smoothing) != 0.0):
        raise NotImplementedError("ohem (online hard example mining) cannot be combined with class_weights / label_smoothing yet: "
                                  "mi_upsample_ce_ohem mines on the plain cross-entropy")


FOCAL_GAMMA_MAX = 8.0          # mi_upsample_ce_focal's range, SOLVER.FOCAL_GAMMA's too


def check_focal_gamma(gamma):
    """The focal exponent as a float in [0, FOCAL_GAMMA_MAX]; 0 = off."""
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError("focal_gamma must be a number in [0, %g], got %r" % (FOCAL_GAMMA_MAX, gamma))
    if not 0.0 <= g <= FOCAL_GAMMA_MAX:          # (a nan fails both comparisons)
        raise ValueError("focal_gamma %r lies outside [0, %g]" % (gamma, FOCAL_GAMMA_MAX))
    return g


def refuse_focal_with(focal_gamma, ohem, label_smoothing):
    """Focal loss (focal_gamma > 0) modulates the hard-label cross-entropy over every valid pixel: every layer refuses it together with OHEM
    or label smoothing with this message.  Returns the checked exponent."""
    g = check_focal_gamma(focal_gamma)
    if g > 0.0 and (ohem is not None or float(label_smoothing) != 0.0):
        raise NotImplementedError("focal_gamma (focal loss) cannot be combined with ohem / label_smoothing: mi_upsample_ce_focal modulates the "
                                  "cross-entropy of the hard labels over every valid pixel (class_weights are fine)")
    return g


class CeCriterion(collections.namedtuple("CeCriterion", "class_weights label_smoothing ohem focal_gamma")):
    """The criterion of a fused upsample + cross-entropy head as one checked value: CrossEntropyLoss's weight= ([K] fp32 on the device, or None) and
    label_smoothing=, OHEM's (thresh, min_kept) or None, the focal exponent (0 = off).  Build it with `of`; upsample_ce_head launches it."""
    __slots__ = ()

    @classmethod
    def of(cls, class_weights=None, label_smoothing=0.0, ohem=None, focal_gamma=0.0):
        """The one place that applies the combination rules (in this order: with everything set, OHEM's refusal is the one reported)."""
        refuse_ohem_with_weights(ohem, class_weights, label_smoothing)
        focal_gamma = refuse_focal_with(focal_gamma, ohem, label_smoothing)
        return cls(class_weights, float(label_smoothing), None if ohem is None else check_ohem(ohem), focal_gamma)


def upsample_ce_focal(low, labels, gamma, want_grad=True, grad_scale=1.0, ignore_index=255, align_corners=True, class_weights=None):
    """Fused upsample + focal loss -w_y (1 - p_y)^gamma log p_y over the valid pixels, divided by their weight sum (mi_upsample_ce_focal).
    Returns (loss_out[4] = loss, S, bad labels, scratch; dlow or None).  class_weights: [K] fp32 on low's device, or None; gamma in [0, 8],
    0 = the weighted cross-entropy's launches and bits."""
    L = _lib.lib()
    dims, ws, out, dlow = _head_buffers(low, labels, L.mi_upsample_ce_workspace, "upce", want_grad)
    gamma = check_focal_gamma(gamma)
    _chk_class_weights(class_weights, low, "upsample_ce_focal")
    check(L.mi_upsample_ce_focal(_p(low), _p(labels), _p(class_weights), _p(out), _p(dlow), *dims, ignore_index, gamma, float(grad_scale),
                                 int(bool(align_corners)), _p(ws), ws.numel(), _stream()), "mi_upsample_ce_focal")
    return out, dlow


def upsample_ce_ohem(low, labels, thresh, min_kept, want_grad=True, grad_scale=1.0, ignore_index=255, align_corners=True, want_prob=False):
    """Fused upsample + cross-entropy over the hard pixels only (OHEM, mi_upsample_ce_ohem): kept = valid and softmax[label] <= t,
    t = max(thresh, min(min_kept, n valid)-th smallest softmax[label]).  Returns (loss_out[4] = loss, n_kept, bad labels, t; dlow or None;
    prob [B,H,W] = softmax[label] of every pixel, 2.0 where it is not valid, or None).  Nothing is read back between its launches."""
    L = _lib.lib()
    dims, ws, out, dlow = _head_buffers(low, labels, L.mi_upsample_ce_ohem_workspace, "upohem", want_grad)
    thresh, min_kept = check_ohem((thresh, min_kept))
    prob = torch.empty(labels.shape, dtype=torch.float32, device=low.device) if want_prob else None
    check(L.mi_upsample_ce_ohem(_p(low), _p(labels), _p(out), _p(dlow), _p(prob), *dims, ignore_index, thresh, min_kept, float(grad_scale),
                                int(bool(align_corners)), _p(ws), ws.numel(), _stream()), "mi_upsample_ce_ohem")
    return out, dlow, prob


def upsample_ce_head(low, labels, crit, want_grad=True, grad_scale=1.0, ignore_index=255, align_corners=True):
    """The fused upsample + cross-entropy head of a CeCriterion: focal_gamma > 0 -> mi_upsample_ce_focal, OHEM -> mi_upsample_ce_ohem, weights or
    smoothing -> mi_upsample_ce_w, else mi_upsample_ce_ex.  Returns (loss_out[4], dlow or None), as the wrapper it calls."""
    kw = {"want_grad": want_grad, "grad_scale": grad_scale, "ignore_index": ignore_index, "align_corners": align_corners}
    if crit.focal_gamma > 0.0:
        return upsample_ce_focal(low, labels, crit.focal_gamma, class_weights=crit.class_weights, **kw)
    if crit.ohem is not None:
        return upsample_ce_ohem(low, labels, *crit.ohem, **kw)[:2]
    return upsample_ce(low, labels, class_weights=crit.class_weights, label_smoothing=crit.label_smoothing, **kw)


GDL_WEIGHT_TYPES = {"square": 0, "identity": 1, "sqrt": 2}          # MI_GDL_* of include/mi355seg.h


def upsample_gdl(low, labels, want_grad=True, grad_scale=1.0, ignore_index=255, weight_type="square", eps=1e-5, align_corners=True, want_sums=False):
    """Fused upsample + GeneralizedDiceLoss (reference utility.py:399-447, label form).  Returns (loss_out[4] = loss, valid pixels, bad labels, 0;
    dlow or None; sums[3K] = T, I, P2 or None).  Nothing is read back between its launches."""
    L = _lib.lib()
    dims, ws, out, dlow = _head_buffers(low, labels, L.mi_upsample_gdl_workspace, "upgdl", want_grad)
    if weight_type not in GDL_WEIGHT_TYPES:
        raise ValueError("Check out the weight_type: %r (one of %s)" % (weight_type, ", ".join(GDL_WEIGHT_TYPES)))
    sums = torch.empty(3 * low.shape[-1], dtype=torch.float32, device=low.device) if want_sums else None
    check(L.mi_upsample_gdl(_p(low), _p(labels), _p(out), _p(dlow), _p(sums), *dims, ignore_index, GDL_WEIGHT_TYPES[weight_type], float(eps),
                            float(grad_scale), int(bool(align_corners)), _p(ws), ws.numel(), _stream()), "mi_upsample_gdl")
    return out, dlow, sums


LOVASZ_BINS = 1024          # the cells of mi_upsample_lovasz's order


def check_lovasz_ce(weight):
    """The weight of the cross-entropy term beside a Lovasz head (SOLVER.LOVASZ_CE) as a finite float >= 0; 0 = the Lovasz head alone."""
    try:
        w = float(weight)
    except (TypeError, ValueError):
        raise ValueError("lovasz must be the weight of the cross-entropy term, a number >= 0, got %r" % (weight,))
    if not 0.0 <= w < float("inf"):          # (a nan fails both comparisons)
        raise ValueError("lovasz: the cross-entropy weight %r is not a finite number >= 0" % (weight,))
    return w


def upsample_lovasz(low, labels, want_grad=True, grad_scale=1.0, ignore_index=255, align_corners=True, want_hist=False, want_err=False):
    """Fused upsample + Lovasz-Softmax (classes present, whole batch) on a 1024-cell order (mi_upsample_lovasz).  Returns (loss_out[4] = loss, valid
    pixels, bad labels, present classes; dlow or None; hist [K,1024,2] int32 = foreground / background pixels per cell, or None; err [B,K,H,W] = the
    kernel's e of every (pixel, class), 2.0 where the pixel is not valid, or None: tests and diagnosis only).  Nothing is read back between its launches."""
    L = _lib.lib()
    dims, ws, out, dlow = _head_buffers(low, labels, L.mi_upsample_lovasz_workspace, "uplovasz", want_grad)
    K = low.shape[-1]
    hist = torch.empty((K, LOVASZ_BINS, 2), dtype=torch.int32, device=low.device) if want_hist else None
    err = torch.empty((low.shape[0], K) + tuple(labels.shape[1:]), dtype=torch.float32, device=low.device) if want_err else None
    check(L.mi_upsample_lovasz(_p(low), _p(labels), _p(out), _p(dlow), _p(hist), _p(err), *dims, ignore_index, LOVASZ_BINS, float(grad_scale),
                               int(bool(align_corners)), _p(ws), ws.numel(), _stream()), "mi_upsample_lovasz")
    return out, dlow, hist, err


class LovaszCriterion(collections.namedtuple("LovaszCriterion", "ce_weight")):
    """The criterion Lovasz-Softmax + ce_weight * cross-entropy of a fused head as one checked value (ce_weight 0: the Lovasz head alone).  Build it
    with `of`; upsample_lovasz_head launches it."""
    __slots__ = ()

    @classmethod
    def of(cls, ce_weight, class_weights=None, label_smoothing=0.0, ohem=None, focal_gamma=0.0):
        """Refuses what the Lovasz term has no place for, instead of ignoring it."""
        if class_weights is not None or float(label_smoothing) != 0.0 or ohem is not None or float(focal_gamma) != 0.0:
            raise NotImplementedError("lovasz (Lovasz-Softmax + cross-entropy) cannot be combined with class_weights / label_smoothing / ohem / focal_gamma: "
                                      "its cross-entropy term is the plain one and the Lovasz term has no class weights")
        return cls(check_lovasz_ce(ce_weight))


def upsample_lovasz_head(low, labels, crit, want_grad=True, grad_scale=1.0, ignore_index=255, align_corners=True):
    """The fused head of a LovaszCriterion: mi_upsample_lovasz and, where ce_weight > 0, mi_upsample_ce_ex on the same low; the two dlow are added at
    the low resolution.  Returns (loss_out[4] = Lovasz + ce_weight * CE, valid pixels, bad labels, present classes; dlow or None), as upsample_ce_head."""
    kw = {"want_grad": want_grad, "grad_scale": grad_scale, "ignore_index": ignore_index, "align_corners": align_corners}
    out, dlow = upsample_lovasz(low, labels, **kw)[:2]
    if crit.ce_weight > 0.0:
        ce_out, ce_dlow = upsample_ce(low, labels, **kw)
        out[0:1].add_(ce_out[0:1], alpha=crit.ce_weight)
        if dlow is not None:
            dlow.add_(ce_dlow, alpha=crit.ce_weight)
    return out, dlow


def upsample_tversky_bce(low, mask, want_grad=True, grad_scale=1.0, alpha=0.7, eps=1.0, weights=(0.5, 0.5), align_corners=False, want_sums=False,
                         phi=None, w_boundary=0.0):
    """Fused upsample + CompoundLoss([TverskyLoss(alpha, eps), BinaryCrossEntropyLoss()], weights) (reference attn/loss.py) for one-channel logits:
    low [B,h,w] fp32, mask [B,H,W] fp32 in [0, 1] (H >= h, W >= w; the same size: no upsample).  Returns (loss_out[4] = loss, tversky, bce, 0;
    dlow [B,h,w] or None; sums[3] = TP, FN, FP or None).  Nothing is read back between its launches.
    phi ([B,H,W] fp32, signed_distance(mask)) adds w_boundary * mean(sigmoid(z) * phi), the boundary loss, through mi_upsample_tversky_bce_sdf:
    loss_out[3] = that mean, sums[4] = TP, FN, FP, sum p phi.  Without phi the call is mi_upsample_tversky_bce as ever (w_boundary must be 0)."""
    if low.dim() != 3 or mask.dim() != 3 or mask.shape[0] != low.shape[0] or mask.device != low.device:
        raise _lib.MiError("upsample_tversky_bce: low [B,h,w] and mask [B,H,W] on one device, got %s on %s and %s on %s"
                           % (tuple(low.shape), low.device, tuple(mask.shape), mask.device))
    if len(weights) != 2:
        raise ValueError("upsample_tversky_bce: weights = (tversky, bce), got %r" % (weights,))
    L = _lib.lib()
    if phi is None:
        if float(w_boundary) != 0.0:
            raise ValueError("upsample_tversky_bce: w_boundary %r needs phi (signed_distance(mask))" % (w_boundary,))
        dims, ws, out, dlow = _head_buffers(low, mask, L.mi_upsample_tversky_bce_workspace, "uptvb", want_grad, torch.float32, "mask")
        sums = torch.empty(3, dtype=torch.float32, device=low.device) if want_sums else None
        check(L.mi_upsample_tversky_bce(_p(low), _p(mask), _p(out), _p(dlow), _p(sums), *dims, float(alpha), float(eps), float(weights[0]),
                                        float(weights[1]), float(grad_scale), int(bool(align_corners)), _p(ws), ws.numel(), _stream()), "mi_upsample_tversky_bce")
        return out, dlow, sums
    _chk(phi, torch.float32, "phi")
    if tuple(phi.shape) != tuple(mask.shape) or phi.device != mask.device:
        raise _lib.MiError("upsample_tversky_bce: phi must be %s on %s like the mask, got %s on %s" % (tuple(mask.shape), mask.device, tuple(phi.shape), phi.device))
    dims, ws, out, dlow = _head_buffers(low, mask, L.mi_upsample_tversky_bce_sdf_workspace, "uptvb", want_grad, torch.float32, "mask")
    sums = torch.empty(4, dtype=torch.float32, device=low.device) if want_sums else None
    check(L.mi_upsample_tversky_bce_sdf(_p(low), _p(mask), _p(phi), _p(out), _p(dlow), _p(sums), *dims, float(alpha), float(eps), float(weights[0]),
                                        float(weights[1]), float(w_boundary), float(grad_scale), int(bool(align_corners)), _p(ws), ws.numel(), _stream()),
          "mi_upsample_tversky_bce_sdf")
    return out, dlow, sums


def signed_distance(mask, thresh=0.5, want_d2=False, want_counts=False):
    """Exact signed Euclidean distance map (mi_signed_distance, the definition: include/mi355seg.h): mask [B,H,W] fp32 on the GPU -> phi [B,H,W] fp32,
    +sqrt(d2) outside G = (mask >= thresh) and -(sqrt(d2) - 1) inside, 0 for an image without a contour.  want_d2 / want_counts (tests and
    diagnosis) return (phi, d2 int32 [B,H,W] or None, counts int32 [B,2] = foreground, background pixels or None) instead.  Nothing is read back."""
    _chk(mask, torch.float32, "mask")
    if mask.dim() != 3:
        raise _lib.MiError("signed_distance: mask must be [B,H,W], got %s" % (tuple(mask.shape),))
    B, H, W = mask.shape
    L = _lib.lib()
    need = L.mi_signed_distance_workspace(B, H, W)
    ws = _workspace(need, mask.device, "sdf")
    phi = torch.empty_like(mask)
    d2 = torch.empty(mask.shape, dtype=torch.int32, device=mask.device) if want_d2 else None
    counts = torch.empty((B, 2), dtype=torch.int32, device=mask.device) if want_counts else None
    check(L.mi_signed_distance(_p(mask), float(thresh), _p(phi), _p(d2), _p(counts), B, H, W, _p(ws), ws.numel() if need else 0, _stream()), "mi_signed_distance")
    return (phi, d2, counts) if (want_d2 or want_counts) else phi


def count_bad_labels(holder, loss_out):
    """Labels outside [0, K) that are not ignore_index are skipped AND counted by the loss kernels (loss_out[2]); torch's CrossEntropyLoss would
    device-assert on them.  Every call's count goes into a persistent device counter `holder.bad_labels` (the kernel zeroes its own per call), which
    the trainer reads once per logging window where it fetches the loss anyway: a bad label in ANY step of the window raises.  The add is issued on
    every call, so it is captured under HIP-graph replay too."""
    bad = holder.__dict__.get("bad_labels")
    if bad is None or bad.device != loss_out.device:
        bad = holder.__dict__["bad_labels"] = torch.zeros(1, dtype=torch.float32, device=loss_out.device)
    bad.add_(loss_out[2:3])


def check_labels(loss_out, num_classes, what="labels"):
    """Raise if the CE kernels saw labels outside [0, num_classes) that are not ignore_index (torch's device assert).
    Synchronises (reads one float): call it where the loss value is fetched anyway."""
    bad = int(loss_out[2].item())
    if bad:
        raise ValueError("%s: %d label values lie outside [0, %d) and are not ignore_index - torch.nn.CrossEntropyLoss would "
                         "raise a device assert; map the label ids to train ids first" % (what, bad, num_classes))


def upsample_softmax(low, size, want_pred=True):
    _chk(low, torch.float32, "low")
    B, h, w, K = low.shape
    H, W = size
    probs = torch.empty((B, K, H, W), dtype=torch.float32, device=low.device)
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=low.device) if want_pred else None
    check(_lib.lib().mi_upsample_softmax(_p(low), _p(probs), _p(pred), B, h, w, K, H, W, _stream()), "mi_upsample_softmax")
    return probs, pred


def upsample_softmax_multi(lows, mirrors, size, div_a, div_b=1.0):
    """Multi-scale, flip-averaged inference tail in one launch: lows = per-source [h,w,K] fp32 NHWC logits (one image each, any sizes),
    mirrors = per-source flags.  Returns ((p_0 + ... + p_{n-1}) / div_a) / div_b as [1,K,H,W] fp32, p_i = softmax(bilinear(low_i -> size)),
    mirrored sources read at column W-1-x (reference multi_scale_inference, utility.py:193-209)."""
    n = len(lows)
    if not 1 <= n <= 16 or len(mirrors) != n:
        raise _lib.MiError("upsample_softmax_multi: 1..16 sources with one mirror flag each (got %d / %d)" % (n, len(mirrors)))
    K = lows[0].shape[-1]
    src = (_lib.MiProbSource * n)()
    for i, (low, m) in enumerate(zip(lows, mirrors)):
        _chk(low, torch.float32, "lows[%d]" % i)
        if low.dim() != 3 or low.shape[-1] != K or low.device != lows[0].device:
            raise _lib.MiError("lows[%d] must be [h,w,%d] on %s, got %s on %s" % (i, K, lows[0].device, tuple(low.shape), low.device))
        src[i].low, src[i].h, src[i].w, src[i].mirror = low.data_ptr(), low.shape[0], low.shape[1], int(bool(m))
    H, W = size
    probs = torch.empty((1, K, H, W), dtype=torch.float32, device=lows[0].device)
    check(_lib.lib().mi_upsample_softmax_multi(ctypes.cast(src, ctypes.c_void_p), n, _p(probs), K, H, W, float(div_a), float(div_b),
                                               _stream()), "mi_upsample_softmax_multi")
    return probs


def upsample_predict_score(lows, mirrors, size, div_a, div_b=1.0, labels=None, ignore_index=255, threshold=0.0, want_pseudo=False, *, class_threshold=None,
                           hist=None):
    """The evaluation tail without the probability map (mi_upsample_predict_score): the per-pixel values of upsample_softmax_multi(lows, mirrors,
    size, div_a, div_b), reduced in registers.  Returns (pred, pseudo, counts): pred uint8 [H,W] = the lowest class index among the maxima,
    pseudo uint8 [H,W] = pred where the maximum >= threshold else 255 (None unless want_pseudo), counts int64 [K*K + 3K] on the device = confusion
    matrix, area_intersection, area_output, area_target of pred against labels [H,W] int64 (None without labels; split_counts names the parts).
    Class-wise pseudo-labels (mi_upsample_predict_score_cw, the same kernel body): class_threshold = K floats on the host (a sequence, an array or
    a CPU tensor) replaces `threshold` in pseudo = pred where the maximum >= class_threshold[pred]; hist = the caller's int64 [K, PSEUDO_BINS]
    device tensor, to which every pixel's (pred, metrics.confidence_bin(maximum)) cell is ADDED - it persists across images."""
    n = len(lows)
    if not 1 <= n <= 16 or len(mirrors) != n:
        raise _lib.MiError("upsample_predict_score: 1..16 sources with one mirror flag each (got %d / %d)" % (n, len(mirrors)))
    K = lows[0].shape[-1]
    dev = lows[0].device
    src = (_lib.MiProbSource * n)()
    for i, (low, m) in enumerate(zip(lows, mirrors)):
        _chk(low, torch.float32, "lows[%d]" % i)
        if low.dim() != 3 or low.shape[-1] != K or low.device != dev:
            raise _lib.MiError("lows[%d] must be [h,w,%d] on %s, got %s on %s" % (i, K, dev, tuple(low.shape), low.device))
        src[i].low, src[i].h, src[i].w, src[i].mirror = low.data_ptr(), low.shape[0], low.shape[1], int(bool(m))
    H, W = size
    counts = None
    if labels is not None:
        _chk(labels, torch.int64, "labels")
        if tuple(labels.shape) != (H, W) or labels.device != dev:
            raise _lib.MiError("labels must be [%d,%d] on %s, got %s on %s" % (H, W, dev, tuple(labels.shape), labels.device))
        counts = torch.zeros(K * K + 3 * K, dtype=torch.int64, device=dev)
    pred = torch.empty((H, W), dtype=torch.uint8, device=dev)
    pseudo = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_pseudo else None
    if class_threshold is None and hist is None:
        check(_lib.lib().mi_upsample_predict_score(ctypes.cast(src, ctypes.c_void_p), n, K, H, W, float(div_a), float(div_b), _p(labels),
                                                   int(ignore_index), float(threshold), _p(pred), _p(pseudo), _p(counts), _stream()),
              "mi_upsample_predict_score")
        return pred, pseudo, counts
    table = None
    if class_threshold is not None:
        values = [float(v) for v in (class_threshold.tolist() if hasattr(class_threshold, "tolist") else class_threshold)]
        if len(values) != K:
            raise _lib.MiError("class_threshold must hold %d values, got %d" % (K, len(values)))
        table = (ctypes.c_float * K)(*values)
    elif want_pseudo:
        raise _lib.MiError("upsample_predict_score: want_pseudo with hist needs class_threshold (the scalar threshold is the plain entry's)")
    bins = 0
    if hist is not None:
        _chk(hist, torch.int64, "hist")
        if hist.dim() != 2 or hist.shape[0] != K or hist.device != dev:
            raise _lib.MiError("hist must be [%d,bins] on %s, got %s on %s" % (K, dev, tuple(hist.shape), hist.device))
        bins = int(hist.shape[1])
    check(_lib.lib().mi_upsample_predict_score_cw(ctypes.cast(src, ctypes.c_void_p), n, K, H, W, float(div_a), float(div_b), _p(labels),
                                                  int(ignore_index), ctypes.cast(table, ctypes.c_void_p) if table is not None else None, _p(pred),
                                                  _p(pseudo), _p(counts), bins, _p(hist), _stream()), "mi_upsample_predict_score_cw")
    return pred, pseudo, counts


def _slide_windows(who, lows, mirror_lows, origins, window, size):
    """The MiSlideWindow array of the sliding-window tails and (n, h, w, K, device).  lows: per-window [h,w,K] fp32 NHWC logits, all of one size;
    mirror_lows: None, or the logits of the mirrored crops, one per window; origins: per-window (y0, x0) in label coordinates; window = (wh, ww)
    label pixels per window; size = (H, W) of the label.  What depends on the geometry (bounds, cover) is the launcher's to refuse."""
    n = len(lows)
    if not 1 <= n <= _lib.SLIDE_MAX_WINDOWS:
        raise _lib.MiError("%s: 1..%d windows (got %d)" % (who, _lib.SLIDE_MAX_WINDOWS, n))
    if len(origins) != n or (mirror_lows is not None and len(mirror_lows) != n):
        raise _lib.MiError("%s: %d windows but %d origins / %s mirror maps" % (who, n, len(origins), "no" if mirror_lows is None else len(mirror_lows)))
    shape, dev = tuple(lows[0].shape), lows[0].device
    if len(shape) != 3:
        raise _lib.MiError("%s: lows[0] must be [h,w,K], got %s" % (who, shape))
    win = (_lib.MiSlideWindow * n)()
    for i in range(n):
        for what, low in (("lows", lows[i]), ("mirror_lows", None if mirror_lows is None else mirror_lows[i])):
            if low is None:
                continue
            _chk(low, torch.float32, "%s[%d]" % (what, i))
            if tuple(low.shape) != shape or low.device != dev:
                raise _lib.MiError("%s[%d] must be %s on %s, got %s on %s" % (what, i, shape, dev, tuple(low.shape), low.device))
        win[i].low = lows[i].data_ptr()
        win[i].low_mirror = None if mirror_lows is None else mirror_lows[i].data_ptr()
        win[i].y0, win[i].x0 = int(origins[i][0]), int(origins[i][1])
    return win, n, shape[0], shape[1], shape[2], dev


def upsample_softmax_slide(lows, mirror_lows, origins, window, size):
    """Sliding-window inference tail in one launch (mi_upsample_softmax_slide): window i covers the label rectangle origins[i] + window; per
    pixel, the windows that contain it contribute softmax(bilinear(low_i -> window)) at its window-local coordinates - averaged with the
    mirrored crop's map read at the mirrored column when mirror_lows is given, as inference(flip=True) does - summed in window order and
    divided by their number.  Returns [1,K,H,W] fp32.  Arguments: _slide_windows."""
    win, n, h, w, K, dev = _slide_windows("upsample_softmax_slide", lows, mirror_lows, origins, window, size)
    H, W = size
    probs = torch.empty((1, K, H, W), dtype=torch.float32, device=dev)
    check(_lib.lib().mi_upsample_softmax_slide(ctypes.cast(win, ctypes.c_void_p), n, h, w, int(window[0]), int(window[1]), _p(probs), K, H, W,
                                               _stream()), "mi_upsample_softmax_slide")
    return probs


def upsample_predict_score_slide(lows, mirror_lows, origins, window, size, labels=None, ignore_index=255, threshold=0.0, want_pseudo=False, *,
                                 class_threshold=None, hist=None):
    """The evaluation tail of upsample_softmax_slide without the probability map (mi_upsample_predict_score_slide).  Returns (pred, pseudo,
    counts) and takes labels, ignore_index, threshold, want_pseudo, class_threshold and hist exactly as upsample_predict_score does: the
    kernel body after the per-pixel values is the same."""
    who = "upsample_predict_score_slide"
    win, n, h, w, K, dev = _slide_windows(who, lows, mirror_lows, origins, window, size)
    H, W = size
    counts = None
    if labels is not None:
        _chk(labels, torch.int64, "labels")
        if tuple(labels.shape) != (H, W) or labels.device != dev:
            raise _lib.MiError("labels must be [%d,%d] on %s, got %s on %s" % (H, W, dev, tuple(labels.shape), labels.device))
        counts = torch.zeros(K * K + 3 * K, dtype=torch.int64, device=dev)
    table = None
    if class_threshold is not None:
        values = [float(v) for v in (class_threshold.tolist() if hasattr(class_threshold, "tolist") else class_threshold)]
        if len(values) != K:
            raise _lib.MiError("class_threshold must hold %d values, got %d" % (K, len(values)))
        table = (ctypes.c_float * K)(*values)
    elif want_pseudo and hist is not None:
        raise _lib.MiError("%s: want_pseudo with hist needs class_threshold (the scalar threshold is the plain tail's)" % who)
    bins = 0
    if hist is not None:
        _chk(hist, torch.int64, "hist")
        if hist.dim() != 2 or hist.shape[0] != K or hist.device != dev:
            raise _lib.MiError("hist must be [%d,bins] on %s, got %s on %s" % (K, dev, tuple(hist.shape), hist.device))
        bins = int(hist.shape[1])
    pred = torch.empty((H, W), dtype=torch.uint8, device=dev)
    pseudo = torch.empty((H, W), dtype=torch.uint8, device=dev) if want_pseudo else None
    check(_lib.lib().mi_upsample_predict_score_slide(ctypes.cast(win, ctypes.c_void_p), n, h, w, int(window[0]), int(window[1]), K, H, W, _p(labels),
                                                     int(ignore_index), float(threshold),
                                                     ctypes.cast(table, ctypes.c_void_p) if table is not None else None, _p(pred), _p(pseudo),
                                                     _p(counts), bins, _p(hist), _stream()), "mi_upsample_predict_score_slide")
    return pred, pseudo, counts


CURVE_BINS = 256            # probability bins per class of the curve tails (include/mi355seg.h)


def _curves_operands(who, K, size, dev, labels, pr, cal):
    """The checks both curve wrappers make on labels [H,W] int64 and the caller's int64 pr [K, 256, 2] / cal [M, 3] (either may be None)."""
    H, W = size
    if labels is None:
        raise _lib.MiError("%s: labels are required" % who)
    _chk(labels, torch.int64, "labels")
    if tuple(labels.shape) != (H, W) or labels.device != dev:
        raise _lib.MiError("labels must be [%d,%d] on %s, got %s on %s" % (H, W, dev, tuple(labels.shape), labels.device))
    if pr is None and cal is None:
        raise _lib.MiError("%s: neither pr nor cal" % who)
    if pr is not None:
        _chk(pr, torch.int64, "pr")
        if tuple(pr.shape) != (K, CURVE_BINS, 2) or pr.device != dev:
            raise _lib.MiError("pr must be [%d,%d,2] on %s, got %s on %s" % (K, CURVE_BINS, dev, tuple(pr.shape), pr.device))
    if cal is not None:
        _chk(cal, torch.int64, "cal")
        if cal.dim() != 2 or cal.shape[1] != 3 or cal.device != dev:
            raise _lib.MiError("cal must be [ece_bins,3] on %s, got %s on %s" % (dev, tuple(cal.shape), cal.device))
    return 0 if cal is None else int(cal.shape[0])


def upsample_curves(lows, mirrors, size, div_a, div_b=1.0, labels=None, *, pr=None, cal=None):
    """Precision-recall and calibration histograms of one picture without the probability map (mi_upsample_curves): from the per-pixel values of
    upsample_softmax_multi(lows, mirrors, size, div_a, div_b) and labels [H,W] int64, what metrics.literal_curves counts is ADDED to the caller's
    int64 device tensors pr [K, 256, 2] and cal [ece_bins, 3] (either may be None; they persist across pictures).  Returns (pr, cal)."""
    n = len(lows)
    if not 1 <= n <= 16 or len(mirrors) != n:
        raise _lib.MiError("upsample_curves: 1..16 sources with one mirror flag each (got %d / %d)" % (n, len(mirrors)))
    K = lows[0].shape[-1]
    dev = lows[0].device
    src = (_lib.MiProbSource * n)()
    for i, (low, m) in enumerate(zip(lows, mirrors)):
        _chk(low, torch.float32, "lows[%d]" % i)
        if low.dim() != 3 or low.shape[-1] != K or low.device != dev:
            raise _lib.MiError("lows[%d] must be [h,w,%d] on %s, got %s on %s" % (i, K, dev, tuple(low.shape), low.device))
        src[i].low, src[i].h, src[i].w, src[i].mirror = low.data_ptr(), low.shape[0], low.shape[1], int(bool(m))
    H, W = size
    M = _curves_operands("upsample_curves", K, (H, W), dev, labels, pr, cal)
    check(_lib.lib().mi_upsample_curves(ctypes.cast(src, ctypes.c_void_p), n, K, H, W, float(div_a), float(div_b), _p(labels), M, _p(pr), _p(cal),
                                        _stream()), "mi_upsample_curves")
    return pr, cal


def upsample_curves_slide(lows, mirror_lows, origins, window, size, labels=None, *, pr=None, cal=None):
    """upsample_curves on the per-pixel values of upsample_softmax_slide (mi_upsample_curves_slide); the windows as in _slide_windows."""
    who = "upsample_curves_slide"
    win, n, h, w, K, dev = _slide_windows(who, lows, mirror_lows, origins, window, size)
    H, W = size
    M = _curves_operands(who, K, (H, W), dev, labels, pr, cal)
    check(_lib.lib().mi_upsample_curves_slide(ctypes.cast(win, ctypes.c_void_p), n, h, w, int(window[0]), int(window[1]), K, H, W, _p(labels), M,
                                              _p(pr), _p(cal), _stream()), "mi_upsample_curves_slide")
    return pr, cal


def split_counts(counts, K):
    """The layout of mi_upsample_predict_score's counts (include/mi355seg.h): (cmt [K,K], intersection [K], output [K], target [K])."""
    return counts[:K * K].reshape(K, K), counts[K * K:K * K + K], counts[K * K + K:K * K + 2 * K], counts[K * K + 2 * K:K * K + 3 * K]


# ---- online self-training: mean teacher + ClassMix (csrc/classmix.hip) -----------------------------------------------------------------------
def label_classes(labels, num_classes, out=None):
    """mi_label_classes: labels [B,H,W] int64 -> present int32 [B] (the uint32 bit set, read as numpy uint32 by tests): bit c set iff class c in
    [0, num_classes) occurs in image b; anything else - the ignore value included - sets nothing.  `out` is overwritten, whatever it held."""
    _chk(labels, torch.int64, "labels")
    if labels.dim() != 3:
        raise _lib.MiError("labels must be [B,H,W], got %s" % (tuple(labels.shape),))
    B, H, W = labels.shape
    present = torch.empty(B, dtype=torch.int32, device=labels.device) if out is None else _chk(out, torch.int32, "present")
    if present.numel() != B or present.device != labels.device:
        raise _lib.MiError("present must hold %d words on %s" % (B, labels.device))
    check(_lib.lib().mi_label_classes(_p(labels), _p(present), B, H, W, int(num_classes), _stream()), "mi_label_classes")
    return present


ClassMix = collections.namedtuple("ClassMix", "image label mask counts")


def classmix(src_img, tgt_img, src_lab, teacher_low, present, priority, threshold, ignore_index=255, out_img=None, out_label=None, want_mask=False):
    """mi_classmix: the pseudo-label and mixing pass without the probability map.  src_img / tgt_img [B,3,H,W] fp32, src_lab [B,H,W] int64,
    teacher_low [B,h,w,K] fp32 NHWC (the teacher's low-resolution logits of tgt_img), present int32 [B] (label_classes of src_lab), priority uint8
    [B,K] on the device (every row a permutation of 0..K-1).  Returns ClassMix(image [B,3,H,W] fp32 - written into out_img when given, which may be a
    contiguous slice of a larger buffer, as out_label may -, label [B,H,W] int64, mask [B,H,W] uint8 or None, counts int64 [B,2] = pasted pixels, kept pseudo-labels
    among the unpasted ones).  Pseudo-labels are bit-equal to upsample_predict_score([teacher_low[b]], [False], (H, W), 1, 1, threshold=...)'s."""
    _chk(src_img, torch.float32, "src_img")
    _chk(tgt_img, torch.float32, "tgt_img")
    _chk(src_lab, torch.int64, "src_lab")
    _chk(teacher_low, torch.float32, "teacher_low")
    _chk(present, torch.int32, "present")
    _chk(priority, torch.uint8, "priority")
    dev = src_img.device
    if src_img.dim() != 4 or src_img.shape[1] != 3 or tgt_img.shape != src_img.shape:
        raise _lib.MiError("src_img and tgt_img must both be [B,3,H,W], got %s and %s" % (tuple(src_img.shape), tuple(tgt_img.shape)))
    B, _, H, W = src_img.shape
    if tuple(src_lab.shape) != (B, H, W):
        raise _lib.MiError("src_lab must be [%d,%d,%d], got %s" % (B, H, W, tuple(src_lab.shape)))
    if teacher_low.dim() != 4 or teacher_low.shape[0] != B:
        raise _lib.MiError("teacher_low must be [%d,h,w,K], got %s" % (B, tuple(teacher_low.shape)))
    _, h, w, K = teacher_low.shape
    if present.numel() != B or tuple(priority.shape) != (B, K):
        raise _lib.MiError("present must hold %d words and priority be [%d,%d], got %s and %s" % (B, B, K, tuple(present.shape), tuple(priority.shape)))
    for t, n in ((tgt_img, "tgt_img"), (src_lab, "src_lab"), (teacher_low, "teacher_low"), (present, "present"), (priority, "priority")):
        if t.device != dev:
            raise _lib.MiError("%s lives on %s, src_img on %s" % (n, t.device, dev))
    if out_img is None:
        out_img = torch.empty_like(src_img)
    else:
        _chk(out_img, torch.float32, "out_img")
        if out_img.shape != src_img.shape or out_img.device != dev:
            raise _lib.MiError("out_img must be %s on %s, got %s on %s" % (tuple(src_img.shape), dev, tuple(out_img.shape), out_img.device))
    if out_label is None:
        out_label = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    else:
        _chk(out_label, torch.int64, "out_label")
        if tuple(out_label.shape) != (B, H, W) or out_label.device != dev:
            raise _lib.MiError("out_label must be [%d,%d,%d] on %s, got %s on %s" % (B, H, W, dev, tuple(out_label.shape), out_label.device))
    label = out_label
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_mask else None
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    check(_lib.lib().mi_classmix(_p(src_img), _p(tgt_img), _p(src_lab), _p(teacher_low), _p(present), _p(priority), float(threshold), int(ignore_index),
                                 _p(out_img), _p(label), _p(mask), _p(counts), B, h, w, K, H, W, _stream()), "mi_classmix")
    return ClassMix(out_img, label, mask, counts)


def ema_update(teacher, student, hyper):
    """mi_ema_update: teacher = a * teacher + (1 - a) * student in place over two flat fp32 tensors of equal length (any 4-byte alignment: views
    into larger buffers are fine), a = hyper[0] read from the device by the kernel (hyper: a one-float device tensor)."""
    for t, n in ((teacher, "teacher"), (student, "student"), (hyper, "hyper")):
        _chk(t, torch.float32, n)
    if teacher.dim() != 1 or teacher.shape != student.shape or hyper.numel() < 1:
        raise _lib.MiError("ema_update: teacher and student must be flat and of one length (got %s and %s), hyper one float" % (tuple(teacher.shape), tuple(student.shape)))
    check(_lib.lib().mi_ema_update(_p(teacher), _p(student), teacher.numel(), _p(hyper), _stream()), "mi_ema_update")


POLYP_SUMS, POLYP_COUNTS = 24, 4            # MI_POLYP_SUMS, MI_POLYP_COUNTS
PolypScore = collections.namedtuple("PolypScore", "hist sums counts prob pred")


def polyp_score(low, labels, want_prob=False, want_pred=True):
    """The polyp evaluation tail (mi_polyp_score): low [B,h,w] fp32 (PraNet's res2 logits), labels [B,H,W] int64 -> PolypScore of device tensors:
    hist int64 [B,2,256] (ground truth x quantised probability), sums float64 [B,24] (the S-measure's quadrant moments, cx, cy, the batch's min /
    max of the sigmoid), counts int64 [B,4] (G, label column / row sums, labels outside {0, 1}), prob fp32 [B,H,W] (the normalised map
    PranetTester.predict thresholds; None unless want_prob) and pred uint8 [B,H,W] (prob > 1 - prob; None unless want_pred).  The statistics are
    the same bits whichever side outputs are asked for.  host/metrics.py polyp_image_stats turns (hist, sums) into the metrics."""
    _chk(low, torch.float32, "low")
    _chk(labels, torch.int64, "labels")
    if low.dim() != 3 or labels.dim() != 3 or labels.shape[0] != low.shape[0] or labels.device != low.device:
        raise _lib.MiError("polyp_score: low [B,h,w] and labels [B,H,W] on one device, got %s on %s and %s on %s"
                           % (tuple(low.shape), low.device, tuple(labels.shape), labels.device))
    (B, h, w), (H, W) = low.shape, labels.shape[1:]
    dev = low.device
    hist = torch.empty((B, 2, 256), dtype=torch.int64, device=dev)
    sums = torch.empty((B, POLYP_SUMS), dtype=torch.float64, device=dev)
    counts = torch.empty((B, POLYP_COUNTS), dtype=torch.int64, device=dev)
    prob = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_prob else None
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_pred else None
    nbytes = _lib.lib().mi_polyp_score_workspace(B, h, w, H, W)
    ws = torch.empty(max(nbytes, 8) // 8 + 1, dtype=torch.float64, device=dev)
    check(_lib.lib().mi_polyp_score(_p(low), _p(labels), B, h, w, H, W, _p(hist), _p(sums), _p(counts), _p(prob), _p(pred), _p(ws), ws.numel() * 8,
                                    _stream()), "mi_polyp_score")
    return PolypScore(hist, sums, counts, prob, pred)


def image_resize_ac(x, size, with_mirror=False):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) on [B,C,H,W] fp32 NCHW; with_mirror appends torch.flip(resized, [3]) of
    image b as image B + b (one launch)."""
    _chk(x, torch.float32, "x")
    B, C, H, W = x.shape
    Ho, Wo = size
    out = torch.empty((B * (2 if with_mirror else 1), C, Ho, Wo), dtype=torch.float32, device=x.device)
    check(_lib.lib().mi_image_resize_ac(_p(x), _p(out), B, C, H, W, Ho, Wo, int(bool(with_mirror)), _stream()), "mi_image_resize_ac")
    return out


CrfResult = collections.namedtuple("CrfResult", "probs pred conf")


def crf_refine(probs, image, cs, iters, window, dilation, pos_w, pos_xy, bi_w, bi_xy, bi_rgb, want_probs=True, want_pred=False, want_conf=False):
    """Locally connected CRF refinement (mi_crf_refine, the definition: include/mi355seg.h): probs [B,K,H,W] fp32 probabilities, image [B,3,H,W]
    fp32 (the normalised input at the same size), cs the three factors from the normalised image to 0..255 units -> CrfResult of device tensors:
    probs fp32 [B,K,H,W] (Q after `iters` mean-field iterations), pred uint8 [B,H,W] (its argmax, lowest index among ties), conf fp32 [B,H,W]
    (its maximum); None where not asked for.  An output's bits do not depend on which others are requested.  1 + iters launches on the current
    stream, workspace cached per stream."""
    _chk(probs, torch.float32, "probs")
    _chk(image, torch.float32, "image")
    if probs.dim() != 4 or image.dim() != 4 or image.shape[1] != 3 or image.shape[0] != probs.shape[0] or image.shape[2:] != probs.shape[2:] \
            or image.device != probs.device:
        raise _lib.MiError("crf_refine: probs [B,K,H,W] and image [B,3,H,W] on one device, got %s on %s and %s on %s"
                           % (tuple(probs.shape), probs.device, tuple(image.shape), image.device))
    cs = [float(v) for v in cs]
    if len(cs) != 3:
        raise _lib.MiError("crf_refine: cs must hold three channel factors, got %d" % len(cs))
    B, K, H, W = probs.shape
    dev = probs.device
    out = torch.empty_like(probs) if want_probs else None
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_pred else None
    conf = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_conf else None
    ws = _workspace(_lib.lib().mi_crf_workspace(B, K, H, W), dev, "crf")
    check(_lib.lib().mi_crf_refine(_p(probs), _p(image), cs[0], cs[1], cs[2], _p(out), _p(pred), _p(conf), B, K, H, W, int(iters), int(window),
                                   int(dilation), float(pos_w), float(pos_xy), float(bi_w), float(bi_xy), float(bi_rgb), _p(ws), ws.numel(),
                                   _stream()), "mi_crf_refine")
    return CrfResult(out, pred, conf)


def boundary_score(pred, labels, num_classes, ignore_index, max_width, hist):
    """Boundary IoU / trimap IoU histograms of one picture (mi_boundary_score, the definition: include/mi355seg.h): pred uint8 [H,W], labels
    int64 [H,W], hist int64 [5, num_classes, max_width + 1] on the same device.  ADDS this picture's counts to hist (the caller zeroes it once
    per data set) and returns it.  Two launches on the current stream, nothing read back; workspace cached per stream."""
    _chk(pred, torch.uint8, "pred")
    _chk(labels, torch.int64, "labels")
    _chk(hist, torch.int64, "hist")
    K, D = int(num_classes), int(max_width)
    if pred.dim() != 2 or labels.shape != pred.shape or labels.device != pred.device or hist.device != pred.device:
        raise _lib.MiError("boundary_score: pred and labels [H,W] on one device with hist, got %s on %s, %s on %s, hist on %s"
                           % (tuple(pred.shape), pred.device, tuple(labels.shape), labels.device, hist.device))
    if tuple(hist.shape) != (5, K, D + 1):
        raise _lib.MiError("boundary_score: hist must be [5, %d, %d], got %s" % (K, D + 1, tuple(hist.shape)))
    H, W = pred.shape
    ws = _workspace(_lib.lib().mi_boundary_score_workspace(H, W), pred.device, "boundary")
    check(_lib.lib().mi_boundary_score(_p(pred), _p(labels), H, W, K, int(ignore_index), D, _p(hist), _p(ws), ws.numel(), _stream()),
          "mi_boundary_score")
    return hist


SURFACE_INTS, SURFACE_MAX_TOL = 27, 8       # MI_SURFACE_INTS, MI_SURFACE_MAX_TOL
SurfaceScore = collections.namedtuple("SurfaceScore", "ints sums")


def surface_tol2(tolerances):
    """floor(tau^2) per tolerance, the integers mi_surface_score compares d2 with (math.floor of the float64 product)."""
    return [int(math.floor(float(t) * float(t))) for t in tolerances]


def surface_score(pred, labels, cls=1, percentile=95, tolerances=(2.0,)):
    """Surface-distance tail (mi_surface_score, the definition: include/mi355seg.h): pred uint8 [B,H,W], labels int64 [B,H,W] on one device ->
    SurfaceScore of device tensors: ints int64 [B,27] (|P|, |G|, |S(P)|, |S(G)|, the two directed maxima of d2, the two order statistics of the
    combined list, floor r, q (n - 1) mod 100, defined, then 2 counts per tolerance) and sums float64 [B,2] (the directed sums of sqrt(d2)).
    Foreground is pred == cls / labels == cls.  host/metrics.py surface_image_stats turns a row of each into HD, HD-q, ASSD and NSD.  Seven
    launches on the current stream, nothing read back; workspace cached per stream."""
    _chk(pred, torch.uint8, "pred")
    _chk(labels, torch.int64, "labels")
    if pred.dim() != 3 or labels.shape != pred.shape or labels.device != pred.device:
        raise _lib.MiError("surface_score: pred and labels [B,H,W] on one device, got %s on %s and %s on %s"
                           % (tuple(pred.shape), pred.device, tuple(labels.shape), labels.device))
    tolerances = tuple(tolerances)
    if len(tolerances) > SURFACE_MAX_TOL or any(not (float(t) >= 0.0 and math.isfinite(float(t))) for t in tolerances):
        raise _lib.MiError("surface_score: at most %d finite, non-negative tolerances, got %r" % (SURFACE_MAX_TOL, tolerances))
    if int(percentile) != percentile:
        raise _lib.MiError("surface_score: the percentile must be an integer in 1..100, got %r" % (percentile,))
    B, H, W = pred.shape
    dev = pred.device
    T = len(tolerances)
    tol2 = (ctypes.c_int32 * max(T, 1))(*surface_tol2(tolerances))
    ints = torch.empty((B, SURFACE_INTS), dtype=torch.int64, device=dev)
    sums = torch.empty((B, 2), dtype=torch.float64, device=dev)
    ws = _workspace(_lib.lib().mi_surface_score_workspace(B, H, W), dev, "surface")
    check(_lib.lib().mi_surface_score(_p(pred), _p(labels), B, H, W, int(cls), int(percentile), ctypes.cast(tol2, ctypes.c_void_p), T, _p(ints), _p(sums),
                                      _p(ws), ws.numel(), _stream()), "mi_surface_score")
    return SurfaceScore(ints, sums)


LESION_INTS = 12                            # MI_LESION_INTS
Components = collections.namedtuple("Components", "labels roots counts")
LesionScore = collections.namedtuple("LesionScore", "ints filtered")


def _chk_components(who, cls, connectivity):
    if int(cls) != cls or not 0 <= int(cls) <= 255:
        raise _lib.MiError("%s: cls must be an integer in 0..255, got %r" % (who, cls))
    if connectivity not in (4, 8):
        raise _lib.MiError("%s: the connectivity must be 4 or 8, got %r" % (who, connectivity))


def label_components(mask, cls=1, connectivity=8, want_labels=True, want_roots=False):
    """Connected components (mi_label_components, the definition: include/mi355seg.h): mask uint8 [B,H,W] -> Components of device tensors:
    labels int32 [B,H,W] (0 on background, else 1..n per image in the raster order of each component's first pixel: scipy.ndimage.label with the
    cross / full 3 x 3 structure), roots int32 [B,H,W] (the linear index of that first pixel, -1 on background) and counts int32 [B].  Foreground
    is mask == cls.  labels / roots are None when not wanted; at least one must be.  Six launches on the current stream, nothing read back;
    workspace cached per stream."""
    _chk(mask, torch.uint8, "mask")
    if mask.dim() != 3:
        raise _lib.MiError("label_components: mask must be [B,H,W], got %s" % (tuple(mask.shape),))
    _chk_components("label_components", cls, connectivity)
    if not (want_labels or want_roots):
        raise _lib.MiError("label_components: at least one of want_labels and want_roots")
    B, H, W = mask.shape
    dev = mask.device
    labels = torch.empty((B, H, W), dtype=torch.int32, device=dev) if want_labels else None
    roots = torch.empty((B, H, W), dtype=torch.int32, device=dev) if want_roots else None
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = _workspace(_lib.lib().mi_label_components_workspace(B, H, W), dev, "components")
    check(_lib.lib().mi_label_components(_p(mask), B, H, W, int(cls), int(connectivity), _p(labels), _p(roots), _p(counts), _p(ws), ws.numel(), _stream()),
          "mi_label_components")
    return Components(labels, roots, counts)


def lesion_permille(overlap):
    """TEST.LESION_OVERLAP as the integer mi_lesion_score compares with."""
    return int(round(1000 * overlap))


def lesion_score(pred, labels, cls=1, connectivity=8, min_area=0, keep_largest=False, overlap=0.0, want_filtered=True):
    """Lesion-wise tail (mi_lesion_score, the definition: include/mi355seg.h): pred uint8 [B,H,W], labels int64 [B,H,W] on one device ->
    LesionScore of device tensors: ints int64 [B,12] (|P|, |P'|, |G|, the components of P, P' and G, the true-positive components of P', the
    detected components of G, the largest component areas of P and G, |P' & G|, the components the filter removed) and filtered uint8 [B,H,W]
    (cls on P', cls == 0 ? 1 : 0 elsewhere; None when not wanted).  P' keeps the components of P = (pred == cls) of at least min_area pixels,
    with keep_largest only the largest; `overlap` in [0, 1] is the share of a component the other mask must cover, as per-mille.
    host/metrics.py lesion_image_stats names the integers.  A memset and seven launches on the current stream, nothing read back; workspace
    cached per stream."""
    _chk(pred, torch.uint8, "pred")
    _chk(labels, torch.int64, "labels")
    if pred.dim() != 3 or labels.shape != pred.shape or labels.device != pred.device:
        raise _lib.MiError("lesion_score: pred and labels [B,H,W] on one device, got %s on %s and %s on %s"
                           % (tuple(pred.shape), pred.device, tuple(labels.shape), labels.device))
    _chk_components("lesion_score", cls, connectivity)
    if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 0:
        raise _lib.MiError("lesion_score: min_area must be an integer >= 0, got %r" % (min_area,))
    if not (isinstance(overlap, (int, float)) and 0.0 <= float(overlap) <= 1.0):
        raise _lib.MiError("lesion_score: the overlap must lie in [0, 1], got %r" % (overlap,))
    B, H, W = pred.shape
    dev = pred.device
    ints = torch.empty((B, LESION_INTS), dtype=torch.int64, device=dev)
    filtered = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_filtered else None
    ws = _workspace(_lib.lib().mi_lesion_score_workspace(B, H, W), dev, "lesion")
    check(_lib.lib().mi_lesion_score(_p(pred), _p(labels), B, H, W, int(cls), int(connectivity), int(min_area), 1 if keep_largest else 0,
                                     lesion_permille(overlap), _p(filtered), _p(ints), _p(ws), ws.numel(), _stream()), "mi_lesion_score")
    return LesionScore(ints, filtered)


def stem_pool_fwd(y, scale, shift):
    """y [B,Hc,Wc,C] bf16 (conv1 output) -> (pool [B,Hp,Wp,C] bf16, idx uint8): FrozenBN + ReLU + maxpool 3x3/2/1."""
    _chk(y, torch.bfloat16, "y")
    B, Hc, Wc, C = y.shape
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    pool = torch.empty((B, Hp, Wp, C), dtype=torch.bfloat16, device=y.device)
    idx = torch.empty((B, Hp, Wp, C), dtype=torch.uint8, device=y.device)
    check(_lib.lib().mi_stem_pool_fwd(_p(y), _p(scale), _p(shift), _p(pool), _p(idx), B, Hc, Wc, C, Hp, Wp, _stream()), "mi_stem_pool_fwd")
    return pool, idx


def stem_pool_bwd(dpool, idx, scale, conv_hw):
    _chk(dpool, torch.bfloat16, "dpool")
    _chk(idx, torch.uint8, "idx")
    B, Hp, Wp, C = dpool.shape
    Hc, Wc = conv_hw
    dy = torch.empty((B, Hc, Wc, C), dtype=torch.bfloat16, device=dpool.device)
    check(_lib.lib().mi_stem_pool_bwd(_p(dpool), _p(idx), _p(scale), _p(dy), B, Hc, Wc, C, Hp, Wp, _stream()), "mi_stem_pool_bwd")
    return dy


def stem_im2col(x, ncols):
    """Patch matrix of the 7x7 / stride 2 / pad 3 stem conv: x [B,3,H,W] bf16 channels_last -> [B,Ho,Wo,ncols] bf16 (147 live columns)."""
    _chk_dtype = x.dtype
    if _chk_dtype != torch.bfloat16 or not x.is_cuda:
        raise _lib.MiError("stem_im2col: x must be a bf16 GPU tensor")
    B, _, H, W = x.shape
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    xn = x.permute(0, 2, 3, 1)
    if not xn.is_contiguous():
        xn = xn.contiguous()
    col = torch.empty((B, Ho, Wo, ncols), dtype=torch.bfloat16, device=x.device)
    check(_lib.lib().mi_stem_im2col(_p(xn), _p(col), B, H, W, Ho, Wo, ncols, _stream()), "mi_stem_im2col")
    return col


def stem_conv_fwd(x, weight):
    """The stem conv as patch matrix + plain GEMM on the implicit-GEMM kernel: returns (y [B,Ho,Wo,64] bf16 NHWC, the patch matrix, which the
    weight gradient reuses)."""
    col = stem_im2col(x, 192)
    O = weight.shape[0]
    wp = torch.zeros((1, O, 192), dtype=torch.bfloat16, device=x.device)
    wp[0, :, :147] = weight.detach().reshape(O, 147).to(torch.bfloat16)
    return conv_gemm(col, wp, (col.shape[1], col.shape[2]), 1, 1, 0, 1, GATHER_FWD), col


def stem_wgrad(dy, x=None, col=None):
    """Weight gradient of the stem conv, deterministic: dy [B,Ho,Wo,64] bf16 NHWC and either the forward's patch matrix `col` or the input
    x [B,3,H,W] bf16 channels_last (a 160-column matrix is built then) -> fp32 [64,3,7,7], by the 1x1 weight-gradient kernel with its
    fixed-order slab reduction."""
    _chk(dy, torch.bfloat16, "dy")
    if col is None:
        col = stem_im2col(x, 160)
    O, n = dy.shape[-1], col.shape[-1]
    dw = torch.empty((O, n, 1, 1), dtype=torch.float32, device=dy.device)
    conv_wgrad(dy, col, dw, 1, 1, 0, 1)
    return dw.view(O, n)[:, :147].reshape(O, 3, 7, 7)


def stem_direct_enabled():
    """MI_STEM_DIRECT (default 1): the stem conv runs on raw image rows (csrc/stem_direct.hip); 0 restores patch matrix + GEMM."""
    return bool(_lib.lib().mi_stem_direct_enabled())


def _stem_out_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


def stem_pack_image(x):
    """x [B,3,H,W] -> bf16 [B,H,W,4] with channel 3 = 0, in one pass: fp32 NCHW-contiguous (the loader's layout) or bf16 channels_last; any other
    dtype / layout is first brought to bf16 channels_last by torch."""
    if not x.is_cuda:
        raise _lib.MiError("stem_pack_image: x must live on the GPU (no CPU path exists)")
    if x.dim() != 4 or x.shape[1] != 3:
        raise _lib.MiError("stem_pack_image: x must be [B,3,H,W], got %s" % (tuple(x.shape),))
    B, _, H, W = x.shape
    if x.dtype == torch.float32 and x.is_contiguous():
        src, nhwc = x, 0
    else:
        src = x.to(dtype=torch.bfloat16).permute(0, 2, 3, 1)
        if not src.is_contiguous():
            src = src.contiguous()
        nhwc = 1
    x4 = torch.empty((B, H, W, 4), dtype=torch.bfloat16, device=x.device)
    check(_lib.lib().mi_stem_pack_image(_p(src), nhwc, _p(x4), B, H, W, _stream()), "mi_stem_pack_image")
    return x4


def stem_conv_direct(x4, weight):
    """The stem conv on the packed image: x4 [B,H,W,4] bf16 (stem_pack_image), weight fp32 [64,3,7,7] -> y [B,Ho,Wo,64] bf16 NHWC (raw conv
    output, bit-equal to stem_conv_fwd's).  No patch matrix: a workgroup stages raw image rows in LDS."""
    _chk(x4, torch.bfloat16, "x4")
    w = _chk(weight.detach(), torch.float32, "weight")
    B, H, W, C4 = x4.shape
    if C4 != 4 or tuple(w.shape[1:]) != (3, 7, 7):
        raise _lib.MiError("stem_conv_direct: x4 %s, weight %s" % (tuple(x4.shape), tuple(w.shape)))
    O = w.shape[0]
    Ho, Wo = _stem_out_hw(H, W)
    y = torch.empty((B, Ho, Wo, O), dtype=torch.bfloat16, device=x4.device)
    wpack = _workspace(6 * 64 * 32 * 2, x4.device, "stem_wpack")
    check(_timed("stem_direct_fwd_kernel", 2.0 * B * Ho * Wo * O * 147, lambda: _lib.lib().mi_stem_conv_fwd(
        _p(x4), _p(w), _p(wpack), _p(y), B, H, W, O, Ho, Wo, _stream()), tag=("fwd", 7, 4, O, B * Ho * Wo, 0, 1)), "mi_stem_conv_fwd")
    return y


def stem_wgrad_direct(dy, x4):
    """Weight gradient of the stem conv on the packed image: dy [B,Ho,Wo,64] bf16 NHWC, x4 [B,H,W,4] bf16 -> fp32 [64,3,7,7]; fixed-order
    partial sums, bit-reproducible."""
    _chk(dy, torch.bfloat16, "dy")
    _chk(x4, torch.bfloat16, "x4")
    B, H, W, C4 = x4.shape
    Ho, Wo = _stem_out_hw(H, W)
    O = dy.shape[-1]
    if C4 != 4 or tuple(dy.shape[:3]) != (B, Ho, Wo):
        raise _lib.MiError("stem_wgrad_direct: dy %s does not belong to x4 %s" % (tuple(dy.shape), tuple(x4.shape)))
    L = _lib.lib()
    dw = torch.empty((O, 3, 7, 7), dtype=torch.float32, device=dy.device)
    ws = _workspace(L.mi_stem_conv_wgrad_workspace(B, Ho, Wo), dy.device, "stem_wgrad")
    check(_timed("stem_direct_wgrad_kernel+reduce", 2.0 * B * Ho * Wo * O * 147, lambda: L.mi_stem_conv_wgrad(
        _p(dy), _p(x4), _p(dw), B, H, W, O, Ho, Wo, _p(ws), ws.numel(), _stream()), tag=("wgrad", 7, 4, O, B * Ho * Wo, 0, 1)), "mi_stem_conv_wgrad")
    return dw


def stem_pool_wgrad_enabled():
    """MI_STEM_POOL_WGRAD (default 1): the direct stem weight gradient builds dy from the pooled gradient inside its launch; 0: stem_pool_bwd first."""
    return bool(_lib.lib().mi_stem_pool_wgrad_enabled())


def stem_wgrad_pool(dpool, idx, scale, x4):
    """stem_wgrad_direct(stem_pool_bwd(dpool, idx, scale, conv size), x4) in one launch, bit-equal, without dy in memory: dpool [B,Hp,Wp,64] bf16
    NHWC, idx uint8 of the same shape (stem_pool_fwd), scale fp32 [64], x4 [B,H,W,4] bf16 -> fp32 [64,3,7,7]."""
    _chk(dpool, torch.bfloat16, "dpool")
    _chk(idx, torch.uint8, "idx")
    _chk(scale, torch.float32, "scale")
    _chk(x4, torch.bfloat16, "x4")
    B, H, W, C4 = x4.shape
    Ho, Wo = _stem_out_hw(H, W)
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    O = dpool.shape[-1]
    if C4 != 4 or tuple(dpool.shape[:3]) != (B, Hp, Wp) or idx.shape != dpool.shape or scale.numel() != O:
        raise _lib.MiError("stem_wgrad_pool: dpool %s / idx %s / scale %s do not belong to x4 %s" % (
            tuple(dpool.shape), tuple(idx.shape), tuple(scale.shape), tuple(x4.shape)))
    L = _lib.lib()
    dw = torch.empty((O, 3, 7, 7), dtype=torch.float32, device=dpool.device)
    ws = _workspace(L.mi_stem_conv_wgrad_workspace(B, Ho, Wo), dpool.device, "stem_wgrad")
    check(_timed("stem_direct_wgrad_kernel<pool>+reduce", 2.0 * B * Ho * Wo * O * 147, lambda: L.mi_stem_conv_wgrad_pool(
        _p(dpool), _p(idx), _p(scale), _p(x4), _p(dw), B, H, W, O, Ho, Wo, Hp, Wp, _p(ws), ws.numel(), _stream()),
        tag=("wgrad", 7, 4, O, B * Ho * Wo, 0, 1)), "mi_stem_conv_wgrad_pool")
    return dw


def head_mask_enabled():
    """MI_HEAD_MASK (default 1): the source-only training step lets the head's data gradient mask the backbone output's gradient in its epilogue."""
    return bool(_lib.lib().mi_head_mask_enabled())


def bias_grad_bf16(dy, db, accumulate=False):
    """db[n] (+)= sum over pixels of dy[..., n];  dy bf16 [B,H,W,N]"""
    _chk(dy, torch.bfloat16, "dy")
    _chk(db, torch.float32, "db")
    N = dy.shape[-1]
    L = _lib.lib()
    ws = _workspace(L.mi_colsum_workspace(dy.numel() // N, N), dy.device, "colsum")
    check(L.mi_bias_grad_bf16(_p(dy), _p(db), dy.numel() // N, N, int(accumulate), _p(ws), ws.numel(), _stream()), "mi_bias_grad_bf16")
    return db


def upsample_softce(seg_low, d_low, size, domain, temperature=1.8, clip=0.9, want_grad=True, grad_scale=1.0):
    """Fused soft-label CE of the FADA step.  seg_low [B,h,w,K] fp32 (detached), d_low [B,h,w,ldD] fp32 (first 2K used).
    Returns (loss_out[2], dd_low or None)."""
    _chk(seg_low, torch.float32, "seg_low")
    _chk(d_low, torch.float32, "d_low")
    B, h, w, Kc = seg_low.shape
    ldD = d_low.shape[-1]
    H, W = size
    L = _lib.lib()
    ws = _workspace(L.mi_upsample_softce_workspace(B, h, w, Kc, H, W), seg_low.device, "softce")
    out = torch.empty(2, dtype=torch.float32, device=seg_low.device)
    dd = torch.empty_like(d_low) if want_grad else None
    check(L.mi_upsample_softce(_p(seg_low), 1.0 / float(temperature), float(clip), _p(d_low), ldD, int(domain), _p(out), _p(dd), B, h, w, Kc,
                               H, W, float(grad_scale), _p(ws), ws.numel(), _stream()), "mi_upsample_softce")
    return out, dd


def upsample_softce_2grid(seg_low, d_low, size, domain, temperature=1.8, clip=0.9, want_grad=True, grad_scale=1.0, seg_align_corners=False,
                          d_align_corners=True):
    """upsample_softce with the two operands on their own grids: seg_low [B,hs,ws,K] fp32 (detached) upsampled with seg_align_corners,
    d_low [B,hd,wd,ldD] fp32 (first 2K used) with d_align_corners, both to `size` (GaldFada: 1/4 and 1/32 resolution).
    Returns (loss_out[2], dd_low or None)."""
    _chk(seg_low, torch.float32, "seg_low")
    _chk(d_low, torch.float32, "d_low")
    B, hs, ws, Kc = seg_low.shape
    Bd, hd, wd, ldD = d_low.shape
    if Bd != B:
        raise _lib.MiError("upsample_softce_2grid: seg_low holds %d images, d_low %d" % (B, Bd))
    H, W = size
    L = _lib.lib()
    ws_buf = _workspace(L.mi_upsample_softce_2grid_workspace(B, hd, wd, Kc, H, W), seg_low.device, "softce2")
    out = torch.empty(2, dtype=torch.float32, device=seg_low.device)
    dd = torch.empty_like(d_low) if want_grad else None
    check(L.mi_upsample_softce_2grid(_p(seg_low), hs, ws, int(bool(seg_align_corners)), 1.0 / float(temperature), float(clip), _p(d_low), hd, wd,
                                     ldD, int(bool(d_align_corners)), int(domain), float(grad_scale), _p(out), _p(dd), B, Kc, H, W, _p(ws_buf),
                                     ws_buf.numel(), _stream()), "mi_upsample_softce_2grid")
    return out, dd


def adam_step(p, g, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_clamp=None):
    for t, n in ((p, "p"), (g, "g"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, torch.float32, n)
    if grad_clamp is not None:          # clip_gradient(optimizer, c) + Adam.step (pranet_trainer.py:59-60): g is clamped in place
        check(_lib.lib().mi_adam_step_clamped(_p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                              int(step), float(grad_clamp), _stream()), "mi_adam_step_clamped")
        return
    check(_lib.lib().mi_adam_step(_p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                  int(step), _stream()), "mi_adam_step")


def adam_step_dev(p, g, exp_avg, exp_avg_sq, hyper):
    """adam_step with (lr, beta1, beta2, eps, grad_clamp or <= 0, step) in a 6-float device tensor (graph-capturable: see mi355seg.h)."""
    for t, n in ((p, "p"), (g, "g"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (hyper, "hyper")):
        _chk(t, torch.float32, n)
    check(_lib.lib().mi_adam_step_dev(_p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), p.numel(), _p(hyper), _stream()), "mi_adam_step_dev")


def sgd_step(p, g, buf, lr, momentum, weight_decay):
    for t, n in ((p, "p"), (g, "g"), (buf, "buf")):
        _chk(t, torch.float32, n)
    check(_lib.lib().mi_sgd_step(_p(p), _p(g), _p(buf), p.numel(), float(lr), float(momentum), float(weight_decay), _stream()),
          "mi_sgd_step")


def sgd_step_dev(p, g, buf, hyper):
    """sgd_step with (lr, momentum, weight_decay) in a 3-float device tensor (graph-capturable: see mi355seg.h)."""
    for t, n in ((p, "p"), (g, "g"), (buf, "buf"), (hyper, "hyper")):
        _chk(t, torch.float32, n)
    check(_lib.lib().mi_sgd_step_dev(_p(p), _p(g), _p(buf), p.numel(), _p(hyper), _stream()), "mi_sgd_step_dev")


def sgd_pack_enabled():
    """MI_SGD_PACK (default 1): FusedSGD's step over a backbone store also writes the bf16 operand packs (sgd_step_pack)."""
    return bool(_lib.lib().mi_sgd_pack_enabled())


def pack_table_gaps(rows, n):
    """[lo, hi) element ranges of a flat store of n floats that no row of a pack table covers (rows: lists [w_off, scale_off, wp_off, wpt_off, O, I, T,
    first_block]), as sgd_step_pack wants them; raises if two rows overlap or one runs past n."""
    gaps, pos = [], 0
    for lo, hi in sorted((int(r[0]), int(r[0]) + int(r[4]) * int(r[5]) * int(r[6])) for r in rows):
        if lo < pos or hi > n:
            raise _lib.MiError("pack table: row [%d, %d) overlaps its neighbour or leaves the store of %d floats" % (lo, hi, n))
        if lo > pos:
            gaps.append([pos, lo])
        pos = hi
    if pos < n:
        gaps.append([pos, n])
    return gaps


def sgd_step_pack(p, g, buf, hyper_or_lr, momentum, weight_decay, sflat, wp, wpt, table_dev, n_desc, total_blocks, gaps_dev):
    """sgd_step (hyper_or_lr a float, with momentum / weight_decay) or sgd_step_dev (hyper_or_lr the 3-float device tensor) over the whole flat store
    plus pack_weights_multi of the updated weights, in one launch (see include/mi355seg.h).  gaps_dev: int64 [n_gaps, 2] on the device
    (pack_table_gaps), or None when the rows cover the store."""
    for t, n in ((p, "p"), (g, "g"), (buf, "buf")):
        _chk(t, torch.float32, n)
    _chk(wp, torch.bfloat16, "wp")
    _chk(table_dev, torch.int64, "table")
    n_gaps = 0 if gaps_dev is None else int(gaps_dev.shape[0])
    if n_gaps:
        _chk(gaps_dev, torch.int64, "gaps")
    L = _lib.lib()
    if torch.is_tensor(hyper_or_lr):
        _chk(hyper_or_lr, torch.float32, "hyper")
        check(L.mi_sgd_step_pack_dev(_p(p), _p(g), _p(buf), p.numel(), _p(hyper_or_lr), _p(sflat), _p(wp), _p(wpt), _p(table_dev), int(n_desc),
                                     int(total_blocks), _p(gaps_dev) if n_gaps else None, n_gaps, _stream()), "mi_sgd_step_pack_dev")
    else:
        check(L.mi_sgd_step_pack(_p(p), _p(g), _p(buf), p.numel(), float(hyper_or_lr), float(momentum), float(weight_decay), _p(sflat), _p(wp), _p(wpt),
                                 _p(table_dev), int(n_desc), int(total_blocks), _p(gaps_dev) if n_gaps else None, n_gaps, _stream()), "mi_sgd_step_pack")


def relu_mask(x, msk, out=None):
    """y = msk > 0 ? x : 0;  msk is a bf16 tensor of x's shape, or packed sign bits (int16, x.numel()/16 words)."""
    _chk(x, torch.bfloat16, "x")
    bits = msk.dtype == torch.int16
    _chk(msk, torch.int16 if bits else torch.bfloat16, "msk")
    if out is None:
        out = torch.empty_like(x)
    check(_lib.lib().mi_relu_mask(_p(x), _p(msk), _p(out), x.numel(), int(bits), _stream()), "mi_relu_mask")
    return out


def frozen_bn_fold(w, b, mean, var):
    for t in (w, b, mean, var):
        _chk(t, torch.float32, "bn buffer")
    scale, shift = torch.empty_like(w), torch.empty_like(w)
    check(_lib.lib().mi_frozen_bn_fold(_p(w), _p(b), _p(mean), _p(var), _p(scale), _p(shift), w.numel(), _stream()),
          "mi_frozen_bn_fold")
    return scale, shift


# ---------------------------------------------------------------------------------------------- PraNet structure loss
def structure_loss(pred, mask, want_grad=True, grad_scale=1.0):
    """pranet_trainer.py:22-31 on fp32 maps [B,1,H,W] (or [B,H,W]): returns (loss scalar tensor, d loss / d pred * grad_scale or None)."""
    _chk(pred, torch.float32, "pred")
    _chk(mask, torch.float32, "mask")
    if pred.shape != mask.shape or (pred.dim() == 4 and pred.shape[1] != 1):
        raise _lib.MiError("structure_loss: pred / mask must be [B,1,H,W] of the same shape, got %s / %s" % (tuple(pred.shape), tuple(mask.shape)))
    B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
    L = _lib.lib()
    ws = torch.empty(int(L.mi_structure_loss_workspace(B, H, W)), dtype=torch.uint8, device=pred.device)
    out = torch.empty(1 + 2 * B, dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    check(L.mi_structure_loss(_p(pred), _p(mask), B, H, W, _p(out), _p(grad), ctypes.c_float(grad_scale), _p(ws), ws.numel(), _stream()),
          "mi_structure_loss")
    return out[0], grad


# ---------------------------------------------------------------------------------------------- trainable BatchNorm2d (NHWC bf16)
_bn_ws = {}


def _bn_workspace(dev, M, C):
    need = int(_lib.lib().mi_bn_workspace(M, C))
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    w = _bn_ws.get(key)
    if w is None or w.numel() < need:
        w = _bn_ws[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return w


def bn_colsum(y, mean=None):
    """Raw per-channel sums over the pixels of a bf16 NHWC tensor: sum y, or sum (y - mean)^2 when `mean` is given."""
    _chk(y, torch.bfloat16, "y")
    C = y.shape[-1]
    M = y.numel() // C
    out = torch.empty(C, dtype=torch.float32, device=y.device)
    ws = _bn_workspace(y.device, M, C)
    _timed("bn_kernels", 0.0, lambda: check(_lib.lib().mi_bn_colsum(_p(y), _p(mean), M, C, _p(out), _p(ws), ws.numel(), _stream()), "mi_bn_colsum"),
           ("bn", 0, C, C, M, 0, 0))
    return out


def bn_colsum2(y, pilot):
    """One pass: raw (sum (y - pilot), sum (y - pilot)^2) per channel - two rows of one [2, C] buffer (one all-reduce when synchronised)."""
    _chk(y, torch.bfloat16, "y")
    C = y.shape[-1]
    M = y.numel() // C
    s1, s2 = torch.empty((2, C), dtype=torch.float32, device=y.device)
    ws = _bn_workspace(y.device, M, C)
    _timed("bn_kernels", 0.0, lambda: check(_lib.lib().mi_bn_colsum2(_p(y), _p(pilot), M, C, _p(s1), _p(s2), _p(ws), ws.numel(), _stream()), "mi_bn_colsum2"),
           ("bn", 4, C, C, M, 0, 0))
    return s1, s2


def bn_finalize(s1, s2, pilot, count, bn):
    """[mean | invstd | gamma * invstd | beta - mean * gamma * invstd] ([4, C] fp32) from the pilot-form sums over `count` pixels, and torch's
    running-statistics update of `bn` (an nn.BatchNorm2d), in one launch."""
    C = s1.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=s1.device)
    track = bn.track_running_stats and bn.running_mean is not None
    if track and bn.momentum is None:
        raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not used by the reference")
    check(_lib.lib().mi_bn_finalize(_p(s1), _p(s2), _p(pilot), float(count), _p(bn.weight.detach()), _p(bn.bias.detach()),
                                    _p(bn.running_mean) if track else None, _p(bn.running_var) if track else None,
                                    _p(bn.num_batches_tracked) if track else None, float(bn.momentum or 0.0), float(bn.eps), _p(out), C, _stream()),
          "mi_bn_finalize")
    return out


def bn_apply(y, mean, scale, beta, res=None, relu=False, want_mask=False):
    """relu?((y - mean) * scale + beta (+ res)) as bf16 NHWC (+ packed sign bits)."""
    _chk(y, torch.bfloat16, "y")
    C = y.shape[-1]
    M = y.numel() // C
    out = torch.empty_like(y)
    bits = torch.empty(y.shape[:-1] + (C // 16,), dtype=torch.int16, device=y.device) if want_mask else None
    _timed("bn_kernels", 0.0, lambda: check(_lib.lib().mi_bn_apply(_p(y), _p(mean), _p(scale), _p(beta), _p(res), _p(out), _p(bits), int(relu), M, C,
                                                                   _stream()), "mi_bn_apply"), ("bn", 1, C, C, M, 0, 0))
    return (out, bits) if want_mask else out


def bn_bwd_colsums(g, y, mean, invstd, relu_bits=None, out=None):
    """Raw (sum g, sum g * xhat) per channel; with relu_bits g counts only where the layer's output was positive.  out: (dbeta, dgamma) to
    write into (the parameters' gradient slots)."""
    _chk(g, torch.bfloat16, "g")
    _chk(y, torch.bfloat16, "y")
    C = y.shape[-1]
    M = y.numel() // C
    if out is None:
        dbeta, dgamma = torch.empty((2, C), dtype=torch.float32, device=y.device)
    else:
        dbeta, dgamma = out
        _chk(dbeta, torch.float32, "dbeta")
        _chk(dgamma, torch.float32, "dgamma")
    ws = _bn_workspace(y.device, M, C)
    _timed("bn_kernels", 0.0, lambda: check(_lib.lib().mi_bn_bwd_colsums(_p(g), _p(y), _p(mean), _p(invstd), _p(relu_bits), M, C, _p(dbeta), _p(dgamma),
                                                                         _p(ws), ws.numel(), _stream()), "mi_bn_bwd_colsums"), ("bn", 2, C, C, M, 0, 0))
    return dbeta, dgamma


def bn_bwd_apply(g, y, mean, invstd, gamma, dbeta, dgamma, count, relu_bits=None):
    """dy of BatchNorm given the (possibly all-reduced) raw sums and the pixel count they were taken over."""
    C = y.shape[-1]
    M = y.numel() // C
    dy = torch.empty_like(y)
    _timed("bn_kernels", 0.0, lambda: check(_lib.lib().mi_bn_bwd_apply(_p(g), _p(y), _p(mean), _p(invstd), _p(gamma), _p(dbeta), _p(dgamma),
                                                                       ctypes.c_float(1.0 / count), _p(relu_bits), _p(dy), M, C, _stream()), "mi_bn_bwd_apply"),
           ("bn", 3, C, C, M, 0, 0))
    return dy


# ---------------------------------------------------------------------------------------------- exact-fp32 evaluation path
def pack_weight_f32(w, out=None):
    """fp32 OIHW -> fp32 [k*k][O][I] (a free view for 1x1)."""
    _chk(w, torch.float32, "w")
    O, I, k, _ = w.shape
    if k == 1:
        return w.detach().view(1, O, I)
    if out is None:
        out = torch.empty((k * k, O, I), dtype=torch.float32, device=w.device)
    check(_lib.lib().mi_pack_weight_f32(_p(w), _p(out), O, I, k, _stream()), "mi_pack_weight_f32")
    return out


def conv_f32(a, wp, out_hw, ksize=1, stride=1, pad=0, dil=1, scale=None, bias=None, res=None, relu=False, out=None):
    """fp32 implicit-GEMM conv on the f32 MFMA: a [B,Ha,Wa,Ca] fp32 NHWC, wp [k*k,N,Ca] fp32 -> [B,Ho,Wo,N] fp32."""
    _chk(a, torch.float32, "a")
    _chk(wp, torch.float32, "wp")
    B, Ha, Wa, Ca = a.shape
    T, N, Cw = wp.shape
    if T != ksize * ksize or Cw != Ca:
        raise _lib.MiError("packed weight %s does not match ksize=%d, Ca=%d" % (tuple(wp.shape), ksize, Ca))
    Ho, Wo = out_hw
    flags = 0
    if bias is not None:
        flags |= EPI_SCALE_BIAS
        _chk(bias, torch.float32, "bias")
        if scale is not None:
            _chk(scale, torch.float32, "scale")
    if res is not None:
        flags |= EPI_RESIDUAL
        _chk(res, torch.float32, "res")
        assert tuple(res.shape) == (B, Ho, Wo, N)
    if relu:
        flags |= EPI_RELU
    if out is None:
        out = torch.empty((B, Ho, Wo, N), dtype=torch.float32, device=a.device)
    _chk(out, torch.float32, "out")
    flops = 2.0 * B * Ho * Wo * N * Ca * ksize * ksize
    check(_timed("igemm_f32_kernel", flops, lambda: _lib.lib().mi_conv_f32(
        _p(a), _p(wp), _p(out), B, Ha, Wa, Ca, Ho, Wo, N, ksize, stride, pad, dil, _p(scale), _p(bias), _p(res), flags, _stream()),
        tag=("f32", ksize, Ca, N, B * Ho * Wo, flags)), "mi_conv_f32")
    return out


def stem_f32(x, w, scale, shift):
    """x [B,3,H,W] fp32 NCHW -> relu(bn(conv7x7/2)) [B,Hc,Wc,64] fp32 NHWC."""
    _chk(x, torch.float32, "x")
    _chk(w, torch.float32, "w")
    B, C, H, W = x.shape
    if C != 3 or tuple(w.shape) != (64, 3, 7, 7):
        raise _lib.MiError("stem_f32 is the 3 -> 64 channel 7x7 stem (got x %s, w %s)" % (tuple(x.shape), tuple(w.shape)))
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Hc, Wc, 64), dtype=torch.float32, device=x.device)
    check(_lib.lib().mi_stem_f32(_p(x), _p(w), _p(scale), _p(shift), _p(y), B, H, W, _stream()), "mi_stem_f32")
    return y


def maxpool_f32(y):
    _chk(y, torch.float32, "y")
    B, Hc, Wc, C = y.shape
    pool = torch.empty((B, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1, C), dtype=torch.float32, device=y.device)
    check(_lib.lib().mi_maxpool_f32(_p(y), _p(pool), B, Hc, Wc, C, _stream()), "mi_maxpool_f32")
    return pool


def augment_batch(table_dev, table_host, B, out_img, out_lab=None):
    """The `aspp` input transform of a batch (include/mi355seg.h, mi_augment_batch): table_dev / table_host hold the same B MiAugSample
    records at their start (device copy, pinned or pageable host copy; host/augment.py builds them), out_img [B,3,h,w] fp32 and
    out_lab [B,lh,lw] fp32 receive the loader contract's tensors.  Enqueued on the current stream."""
    _chk(out_img, torch.float32, "out_img")
    if not table_dev.is_cuda or table_host.is_cuda or table_dev.dtype != torch.uint8 or table_host.dtype != torch.uint8:
        raise _lib.MiError("augment_batch: table_dev is a uint8 device tensor and table_host its uint8 host copy")
    need = B * ctypes.sizeof(_lib.MiAugSample)
    if table_dev.numel() < need or table_host.numel() < need or out_img.dim() != 4 or out_img.shape[0] != B or out_img.shape[1] != 3:
        raise _lib.MiError("augment_batch: %d records need %d bytes of table, out_img must be [%d,3,h,w]" % (B, need, B))
    lh = lw = 0
    if out_lab is not None:
        _chk(out_lab, torch.float32, "out_lab")
        if out_lab.dim() != 3 or out_lab.shape[0] != B:
            raise _lib.MiError("augment_batch: out_lab must be [%d,lh,lw]" % B)
        lh, lw = out_lab.shape[1], out_lab.shape[2]
    check(_lib.lib().mi_augment_batch(_p(table_dev), _p(table_host), B, out_img.shape[2], out_img.shape[3], lh, lw, _p(out_img), _p(out_lab),
                                      _stream()), "mi_augment_batch")
    return out_img, out_lab


def augment_pra_batch(table_dev, table_host, B, out_img, out_mask=None):
    """The `pra` input transform of a batch (include/mi355seg.h, mi_augment_pra_batch): table_dev / table_host hold the same B MiPraSample
    records at their start (host/pra_augment.py builds them), out_img [B,3,h,w] fp32 and out_mask [B,h,w] fp32 receive the loader
    contract's tensors.  Enqueued on the current stream."""
    _chk(out_img, torch.float32, "out_img")
    if not table_dev.is_cuda or table_host.is_cuda or table_dev.dtype != torch.uint8 or table_host.dtype != torch.uint8:
        raise _lib.MiError("augment_pra_batch: table_dev is a uint8 device tensor and table_host its uint8 host copy")
    need = B * ctypes.sizeof(_lib.MiPraSample)
    if table_dev.numel() < need or table_host.numel() < need or out_img.dim() != 4 or out_img.shape[0] != B or out_img.shape[1] != 3:
        raise _lib.MiError("augment_pra_batch: %d records need %d bytes of table, out_img must be [%d,3,h,w]" % (B, need, B))
    if out_mask is not None:
        _chk(out_mask, torch.float32, "out_mask")
        if tuple(out_mask.shape) != (B, out_img.shape[2], out_img.shape[3]):
            raise _lib.MiError("augment_pra_batch: out_mask must be [%d,%d,%d]" % (B, out_img.shape[2], out_img.shape[3]))
    check(_lib.lib().mi_augment_pra_batch(_p(table_dev), _p(table_host), B, out_img.shape[2], out_img.shape[3], _p(out_img), _p(out_mask), _stream()),
          "mi_augment_pra_batch")
    return out_img, out_mask
