"""The tape engine of the general-conv networks (PraNet: host/pranet.py, GALD: host/gald.py): a module's forward AND backward as a schedule of
C-ABI launches (csrc/gconv.hip, gnet.hip).  Unit / Var / Run are what a net's graph is written against, Engine is the nn.Module that stores
its parameters and runs it as one autograd node, FlatAdam updates the whole module in one launch.

Design.  Activations are NHWC bf16; `torch.split` / `torch.cat` of the reference are channel-slice views of one buffer (a conv reads its
26-channel group in place and its BatchNorm writes straight into the concatenation the next conv reads).  Every BatchNorm2d runs on
batch statistics in train(): the conv's epilogue emits per-tile sums, `mi_gbn_finalize` turns them into mean / invstd / folded affine
and updates the running statistics, `mi_gbn_apply` normalises (+ ReLU, + residual).  The backward pass is a tape of closures recorded
by the forward, replayed in reverse: BatchNorm backward sums + apply, weight gradient into the parameter's slot of ONE flat fp32
gradient buffer (clamped Adam updates it in one launch), data gradient.  The one-channel side maps are fp32.  No tensor visits the CPU.
"""
import math
import os

import torch
import torch.nn as nn

from .. import _lib
from .. import gk
from .. import kernels as K
from . import arch
from .engine import FlatStore, WgradScheduler


class Unit:
    """One conv (+ its BatchNorm2d): parameter handles, geometry (kh, kw, sh, sw, ph, pw, dh, dw), packed-operand views."""
    __slots__ = ("key", "bnkey", "cin", "cout", "geom", "weight", "bn", "bias", "wp", "wpt", "depthwise")

    def __init__(self, key, bnkey, cin, cout, k, stride=1, pad=0, dil=1):
        kh, kw = (k, k) if isinstance(k, int) else k
        ph, pw = (pad, pad) if isinstance(pad, int) else pad
        self.key, self.bnkey, self.cin, self.cout = key, bnkey, cin, cout
        self.geom = (kh, kw, stride, stride, ph, pw, dil, dil)
        self.weight = self.bn = self.bias = self.wp = self.wpt = None
        self.depthwise = False          # bias: None, or True before registration = "this conv carries a bias" (set by the architecture tables)


SIDE_MIN_WORK = 8e9          # weight gradients at least this large go to the side stream one by one (GALD: flat from 2 to 16 GFLOP; none: -3 %)
# the queue keeps every dy alive (and its flush sums a private split-K slab per job): bounded, so that backward's peak memory does not grow with the depth
# of the net - 2048 MB of queued gradients (PraNet at 16 x 352 x 352 and GALD at 6 x 720 x 1280 never reach it; a flush costs one more pair of launches)
_WQ_BUDGET = 2048 << 20
# With a side stream (GALD) the queue is flushed every few convs, so that the table-driven launches run beside the data-gradient chain instead of alone at the end
# of the tape: 4 jobs per launch 176.8 images/s, 8: 175.9, 2: 175.3, 16: 174.0, only at the end: 172.1 (one box, two rounds)
_WQ_SIDE_JOBS = 4


# ------------------------------------------------------------------------------------------------ tape
class Var:
    """A tensor of the schedule with its gradient slot.  `own`: the gradient tensor belongs to this variable alone (in-place accumulation is
    safe); `want`: where the gradient should be assembled (a channel slice of the parent's gradient buffer)."""
    __slots__ = ("t", "g", "own", "want", "needs")

    def __init__(self, t, needs=True):
        self.t, self.g, self.own, self.want, self.needs = t, None, False, None, needs


def acc(v, t, own):
    if not v.needs:
        return
    if v.g is None:
        if v.want is not None:
            if t.data_ptr() != v.want.data_ptr():
                gk.gbinary(gk.OP_COPY, t, out=v.want)
            v.g, v.own = v.want, True
        else:
            v.g, v.own = t, own
    elif v.own:
        gk.gbinary(gk.OP_ADD, v.g, t, out=v.g)
    else:
        v.g, v.own = gk.gbinary(gk.OP_ADD, v.g, t), True


def rup32(c):
    return (c + 31) // 32 * 32


_TILE_MIN_PIXELS = 16384          # below this the MFMA-tile kernels do not fill the chip (4096 measured: GALD 169.1 vs 170.1, PraNet 1040 vs 1046 images/s)


def tile_route(u, pixels):
    """Geometry half of mfma_tile_ok: a conv whose shape the implicit-GEMM kernels of the DeepLab path can take (csrc/igemm_nt.hip / igemm_pp.hip /
    igemm_tn.hip: 128 .. 320-row MFMA tiles, LDS-DMA staging, 4x the throughput of the general kernel on large shapes): square 1x1 / 3x3 taps with one
    stride / padding / dilation, enough pixels to fill the chip, and channel counts that are either 64-multiples on both sides or - stride 1 - pad to
    32-multiples with less than 1.6x the work (HarDNet's gathered layers, 466 -> 168 as 480 -> 192: the general kernel's packs are zero-padded to 32 on
    both sides, i.e. they ARE the [taps][N][Ca] operands of those kernels for the padded shape; round 5) - unless the padded Cin is no 64-multiple AND the
    layer has fewer than 192 output columns: such a launch can only take the 256-column main loop and would leave most of it empty (152 -> 58, 218 -> 78)."""
    kh, kw, sh, sw, ph, pw, dh, dw = u.geom
    if u.depthwise or kh != kw or kh not in (1, 3) or sh != sw or ph != pw or dh != dw or pixels < _TILE_MIN_PIXELS:
        return False
    if u.cin % 64 == 0 and u.cout % 64 == 0:
        return True
    ci, co = rup32(u.cin), rup32(u.cout)
    work = 2.0 * pixels * u.cin * u.cout * kh * kw              # the small ones stay where they are: nothing to win on a 5 GFLOP launch
    if ci % 64 and co < 192:      # a padded Cin that only the 256-column main loop takes (mi_conv_gemm: Ca % 64 != 0), with too few output columns to fill it
        return False
    return sh == 1 and 2 * ph == dh * (kh - 1) and work >= 8e9 and ci * co < 1.6 * u.cin * u.cout and os.environ.get("MI_TILE_PAD", "1") != "0"


def mfma_tile_ok(u, x, out=None, out_f32=False):
    """The conv goes to the MFMA-tile kernels: tile_route() and an input that IS the kernels' operand - a contiguous NHWC tensor of the 32-padded channel
    count (64-multiples: the tensor itself; otherwise a gather buffer its producer allocated padded, pad channels zero: gald._hard_block)."""
    if out_f32 or not tile_route(u, x.shape[0] * x.shape[1] * x.shape[2]) or x.shape[-1] != rup32(u.cin):
        return False
    return x.is_contiguous() and (out is None or (out.is_contiguous() and out.shape[-1] == rup32(u.cout)))


def _conv_forward(x, u, bias, stats, out=None, out_f32=False, net=None):
    """(y, statistics partials or None): the general kernel, or the MFMA-tile kernels with the BatchNorm sums out of their epilogue (mi_conv_gemm_stats;
    one extra pass of column sums where a bias or a slot output rules that entry out).  With padded channel counts y is the [.., :cout] view of the
    kernels' 32-padded output (pad columns: products with the pack's zero rows)."""
    if not mfma_tile_ok(u, x, out, out_f32):
        return gk.gconv(x, u.wp, u.cout, u.geom, out=out, bias=bias, stats=stats, out_f32=out_f32)
    k, s, p, d = u.geom[0], u.geom[2], u.geom[4], u.geom[6]
    hw = gk.conv_out_hw(x.shape[1], x.shape[2], *u.geom)
    np_, cp = rup32(u.cout), rup32(u.cin)
    wp = u.wp.view(k * k, np_, cp)
    cut = (lambda t: t) if np_ == u.cout else (lambda t: t[..., :u.cout])
    if stats and bias is None and out is None:          # sum y and sum y^2 out of the conv's own epilogue (pilot 0: raw sums)
        y, sums, _ = K.conv_gemm_stats(x, wp, hw, k, s, p, d, net._zeros(np_))
        return cut(y), (sums if np_ == u.cout else sums[:, :u.cout].contiguous()).view(-1)
    if bias is not None and np_ != u.cout:
        bias = torch.cat([bias, bias.new_zeros(np_ - u.cout)])
    y = cut(K.conv_gemm(x, wp, hw, k, s, p, d, K.GATHER_FWD, scale=None if bias is None else net._ones(np_), bias=bias, out=out))
    st = None
    if stats:                       # sum y and sum y^2 in one pass: the backward-sums kernel with g = y, mean = 0, invstd = 1
        st = torch.empty((2, u.cout), dtype=torch.float32, device=x.device)
        gk.gbn_bwd_sums(y, y, None, net._zeros(u.cout), net._ones(u.cout), st[0], st[1])
        st = st.view(-1)
    return y, st


def grad_target(v):
    """Where a kernel may write d loss / d v directly: the assembly slot if there is one and nothing has been written yet."""
    return v.want if (v.want is not None and v.g is None) else None


class _WgradQueue:
    """Where and when the tape's weight gradients run, on a WgradScheduler (with a side stream when the run class's WGRAD_STREAM asks for one).
    General-kernel weight gradients below SIDE_MIN_WORK, and the image's, are queued and run as one table-driven launch - alone each is a 25 - 60 us
    latency chain of which 15 - 25 us are fixed; the rest are written directly, on the side stream or inline.  The accumulate flags come from tape
    order, so two rules hold for every write to a gradient slot, whatever its route: a slot with a queued job is flushed before anything else writes
    it, and an inline write to a slot that the side stream has written since the last join waits for the side stream first."""

    def __init__(self, sched):
        self.sched = sched
        self.jobs, self.queued, self.beside, self.bytes = [], set(), set(), 0

    def _claim(self, slot, on_side):
        key = slot.data_ptr()
        if key in self.queued:
            self.flush()
        if on_side:
            self.beside.add(key)
        elif key in self.beside:
            self.sched.join()
            self.beside.clear()

    def direct(self, slot, fn, dy, x, side):
        """fn() writes `slot` now: on the side stream (side: True) or inline."""
        self._claim(slot, side)
        self.sched.run(fn, dy, x) if side else fn()

    def put(self, dy, x, slot, geom, acc, cin):
        """Queue slot (+)= the weight gradient of (dy, x), keeping dy and x alive until the flush.  cin: x is the zero-padded image, whose gradient
        for all its channels goes to scratch that the flush allocates on the stream that runs it, the real `cin` cut out after (else None)."""
        self._claim(slot, self.sched.side is not None)
        self.jobs.append((dy, x, slot, geom, acc, cin))
        self.queued.add(slot.data_ptr())
        self.bytes += dy.numel() * dy.element_size()
        if self.bytes > _WQ_BUDGET or (self.sched.side is not None and len(self.jobs) >= _WQ_SIDE_JOBS):
            self.flush()

    def flush(self):
        jobs = self.jobs
        if not jobs:
            return
        if self.sched.side is not None:
            self.beside |= self.queued
        self.jobs, self.queued, self.bytes = [], set(), 0

        def go():
            table, fix = [], []
            for dy, x, slot, geom, acc, cin in jobs:
                if cin is None:
                    table.append((dy, x, slot, geom, acc))
                else:
                    wide = torch.empty((slot.shape[0], x.shape[-1]) + tuple(geom[:2]), dtype=torch.float32, device=dy.device)
                    table.append((dy, x, wide, geom, False))
                    fix.append((slot, wide[:, :cin], acc))
            gk.gconv_wgrad_multi(table)
            for slot, real, acc in fix:
                slot.add_(real) if acc else slot.copy_(real)
        # with a side stream (GALD) the table-driven launch runs beside the data-gradient chain that is still being enqueued
        self.sched.run(go, *[t for j in jobs for t in j[:2]])


class Run:
    """One forward pass.  train: BatchNorm2d on batch statistics (module.training); rec: record the backward tape."""
    WGRAD_STREAM = False          # the large weight gradients of backward() on the side stream (see _conv_backward)

    def __init__(self, net, train, rec):
        self.net, self.train, self.rec, self.tape = net, train, rec, []
        self.wq = None                  # the weight-gradient queue of backward() (_WgradQueue)
        # MI_APPLY_MULTI=0: every gather copy / hierarchical add as its own launch again (the BatchNorm apply then has one destination; same bits)
        self.multi = os.environ.get("MI_APPLY_MULTI", "1") != "0"
        # fp32: the evaluation forward in the reference's precision (csrc/gf32.hip; Engine.set_precision): every activation fp32, every conv with
        # its eval()-BatchNorm affine, residual and activation in one launch
        self.f32 = (not train) and getattr(net, "precision", "bf16") == "fp32"
        if self.f32 and rec:
            raise _lib.MiError("precision 'fp32' is the evaluation forward (no backward kernels exist in fp32): run under torch.no_grad(), or set_precision('bf16')")

    def record(self, fn):
        if self.rec:
            self.tape.append(fn)

    def var(self, t, needs=True):
        return Var(t, needs and self.rec)

    def node(self, t, back):
        """The variable of t; on replay back(g) runs iff a gradient reached it, and the variable lets go of g first."""
        ov = self.var(t)
        if self.rec:
            def replay():
                g = ov.g
                if g is not None:
                    ov.g = None
                    back(g)
            self.tape.append(replay)
        return ov

    def tap(self, name, v):
        """Named intermediates.  A module with a `_taps` dict keeps them (tools/dbg, tests).  Teacher forcing (tests): a module with a `_force` dict
        has the named activations REPLACED in place - after the engine's own value went to `_taps` - by the given tensors, and one with a
        `_force_grad` dict has d loss / d (that activation) replaced - after the engine's own accumulated gradient went to `_gtaps` - before the
        producer's backward runs.  The tests feed every block the oracle's activation and upstream gradient and compare what the block makes of
        them with the oracle's next activation / gradients: an error is attributed to the block that makes it instead of being amplified through
        the rest of the net.  Forced tensors are NCHW (any float dtype, on the module's device)."""
        net = self.net
        taps, force = getattr(net, "_taps", None), getattr(net, "_force", None)
        if force is not None and name in force:
            if taps is not None:
                taps[name] = Var(v.t.clone(), False)
            f = force[name]
            v.t.copy_(f.permute(0, 2, 3, 1) if f.dim() == 4 else f)
        elif taps is not None:
            taps[name] = v
        gtaps, fgrad = getattr(net, "_gtaps", None), getattr(net, "_force_grad", None)
        if self.rec and (gtaps is not None or fgrad is not None):
            def back():                 # runs after every consumer's backward and before the producer's
                if gtaps is not None and v.g is not None:
                    gtaps[name] = v.g.clone()
                if fgrad is not None and name in fgrad:
                    f = fgrad[name]
                    f = (f.permute(0, 2, 3, 1) if f.dim() == 4 else f).to(v.t.dtype)
                    if v.want is not None:
                        v.want.copy_(f)
                        v.g, v.own = v.want, True
                    else:
                        v.g, v.own = f.contiguous(), True
            self.record(back)
        return v

    # ---- conv (+ bias) + BatchNorm2d (+ add) (+ ReLU | ReLU6): BasicConv2d of PraNet_Res2Net.py:7-20, the conv/bn pairs of Res2Net_v1b.py,
    #      ConvLayer of hardnet_68.py:56-80 (relu=6), the conv(bias)-bn-relu stems of FAM (gcpa_gald.py:84-86)
    def _apply(self, y, sc, sh, act, add, out, out_f32, extras):
        """BatchNorm apply; `extras` = [(c0, c1, dst, add2 Var or None), ...]: channel ranges of the result that also go elsewhere in the same launch."""
        if not extras:
            return gk.gbn_apply(y, sc, sh, act, add=add, out=out, out_f32=out_f32)
        return gk.gbn_apply_multi(y, sc, sh, act, [(c0, c1, d, None if a2 is None else a2.t) for c0, c1, d, a2 in extras], add=add, out=out)

    def conv_bn(self, x, u, relu, add=None, out=None, out_f32=False, extras=None):
        if relu == 6 and add is not None:
            # the residual's backward masks with OP_RELU_MASK (out > 0), which would keep the gradient where ReLU6 clamped to 6; no layer needs the pair
            raise _lib.MiError("conv_bn: ReLU6 together with a residual add is not supported")
        net, bn = self.net, u.bn
        act = 2 if relu == 6 else int(bool(relu))
        bias = None if u.bias is None else u.bias.detach()
        if extras and out_f32:
            raise _lib.MiError("conv_bn: extra destinations go with a bf16 output")
        if not self.train:
            sc, sh = net._eval_fold(u)
            if self.f32:
                o = gk.gconv_f32(x.t, u.weight.detach(), u.geom, bias=bias, scale=sc, shift=sh, add=None if add is None else add.t, relu=relu, out=out)
                for c0, c1, d, a2 in (extras or ()):          # fp32 evaluation: the extra destinations as their own element-wise launches
                    gk.gbinary(gk.OP_COPY, o[..., c0:c1], out=d) if a2 is None else gk.gbinary(gk.OP_ADD, o[..., c0:c1], a2.t, out=d)
                return self.var(o, False)
            y, _ = _conv_forward(x.t, u, bias, False, net=net)
            return self.var(self._apply(y, sc, sh, act, None if add is None else add.t, out, out_f32, extras), False)
        hw = gk.conv_out_hw(x.t.shape[1], x.t.shape[2], *u.geom)
        if not mfma_tile_ok(u, x.t) and gk.gconv_bn_fits(x.t.shape[0], *hw) and os.environ.get("MI_BN_INLAUNCH", "0") == "1":
            # small maps, opt-in (MI_BN_INLAUNCH=1): the conv's last workgroup finalizes the statistics itself (one launch instead of two; the same bits).
            # Off by default since round 5: under the HIP-graph replay PraNetTrainer runs it costs 1 % (1 035 vs 1 045 images/s, profiles/r05_inlaunch_ab.txt)
            y, fin = gk.gconv_bn(x.t, u.wp, u.cout, u.geom, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, bias=bias)
            M = y.shape[0] * y.shape[1] * y.shape[2]
        else:
            y, st = _conv_forward(x.t, u, bias, True, net=net)
            M = y.shape[0] * y.shape[1] * y.shape[2]
            fin = gk.gbn_finalize(st, u.cout, M, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)      # mean, invstd, scale, shift
        o = self._apply(y, fin[2], fin[3], act, None if add is None else add.t, out, out_f32, extras)

        def back(g):
            mask = None
            if add is not None:
                if act:
                    g = gk.gbinary(gk.OP_RELU_MASK, g, o)
                acc(add, g, False)
            elif act:
                mask = o
            (dbeta, a1), (dgamma, a2) = net._grad_slot(bn.bias), net._grad_slot(bn.weight)
            if a1 != a2:
                raise _lib.MiError("BatchNorm weight / bias gradient slots out of step")
            gk.gbn_bwd_sums(g, y, mask, fin[0], fin[1], dbeta, dgamma, accumulate=a1, relu6=act == 2)
            if a1:          # a module applied twice (shared parameters): this application's own sums, not the accumulated ones, enter its dy
                db1, dg1 = torch.empty_like(dbeta), torch.empty_like(dgamma)
                gk.gbn_bwd_sums(g, y, mask, fin[0], fin[1], db1, dg1, relu6=act == 2)
            else:
                db1, dg1 = dbeta, dgamma
            dyp = None
            if u.cout % 32 and mfma_tile_ok(u, x.t):
                # the MFMA-tile kernels contract over the 32-padded channel count: d loss / d y goes into the real columns of a padded tensor, pads zero
                dyp = gk.new(y.shape[0], y.shape[1], y.shape[2], rup32(u.cout), y.device)
                dyp[..., u.cout:].zero_()
            dy = gk.gbn_bwd_apply(g, y, mask, fin[0], fin[1], bn.weight, db1, dg1, M, out=None if dyp is None else dyp[..., :u.cout], relu6=act == 2)
            if u.bias is not None:
                slot, accum = net._grad_slot(u.bias)
                gk.gbn_bwd_sums(dy, None, None, None, None, slot, None, accumulate=accum)
            self._conv_backward(x, u, dy if dyp is None else dyp)
        return self.node(o, back)

    def _conv_backward(self, x, u, dy):
        """Weight gradient (off the critical path, _WgradQueue: nothing reads it before the optimizer, and the convs of these nets are far too small to
        fill 256 CUs alone) and data gradient."""
        slot, accum = self.net._grad_slot(u.weight)
        q = self.wq
        # The run class's WGRAD_STREAM (off for PraNet, on for GALD) gives the queue its side stream.  Measured: every weight gradient on the side stream costs
        # PraNet 6 % as a graph and 18 % eager (hundreds of 20-60 us launches, each fork / join a dependency the GPU has to resolve); only the launches of
        # >= 8 GFLOP there: PraNet still -10 % as a graph (659 vs 734 images/s: a second stream in the capture changes how the whole graph is scheduled),
        # GALD (eager, its decoder's and padded gathers' weight gradients are 100 - 400 us launches) +1.5 % (175.6 vs 173.0 images/s, round 5)
        work = 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * u.cout * (1 if u.depthwise else u.cin) * u.geom[0] * u.geom[1]
        side = q.sched.side is not None and work >= SIDE_MIN_WORK
        if mfma_tile_ok(u, x.t) and dy.is_contiguous() and dy.shape[-1] == rup32(u.cout):
            k, s, p, d = u.geom[0], u.geom[2], u.geom[4], u.geom[6]
            np_, cp = rup32(u.cout), rup32(u.cin)
            def wgrad(dw, accumulate):
                # on the side stream the launch runs beside the data-gradient chain: the deferred-reducer form plans its split for that (mi_conv_wgrad_partial)
                if side:                                 # (GALD: 176.6 vs 175.9 images/s)
                    b = K.WgradBatch()
                    K.conv_wgrad(dy, x.t, dw, k, s, p, d, accumulate=accumulate, batch=b)
                    b.flush()
                else:
                    K.conv_wgrad(dy, x.t, dw, k, s, p, d, accumulate=accumulate)
            def padded_wgrad():         # padded operands: the gradient of the padded weight, its real corner into the parameter's slot
                wide = torch.empty((np_, cp, k, k), dtype=torch.float32, device=dy.device)
                wgrad(wide, False)
                slot.add_(wide[:u.cout, :u.cin]) if accum else slot.copy_(wide[:u.cout, :u.cin])
            q.direct(slot, (lambda: wgrad(slot, accum)) if np_ == u.cout and cp == u.cin else padded_wgrad, dy, x.t, side)
            if x.needs:
                tgt = grad_target(x)
                dx = K.conv_gemm(dy, u.wpt.view(k * k, cp, np_), (x.t.shape[1], x.t.shape[2]), k, s, p, d, K.GATHER_DGRAD,
                                 out=tgt if (tgt is not None and tgt.is_contiguous() and tgt.shape[-1] == cp) else None)
                acc(x, dx, True)
            return
        padded = x.t.shape[-1] != u.cin and not u.depthwise              # the zero-padded image (_nhwc_input)
        if side and not padded:
            q.direct(slot, lambda: gk.gconv_wgrad(dy, x.t, slot, u.geom, accumulate=accum), dy, x.t, True)
        else:
            q.put(dy, x.t, slot, u.geom, accum, u.cin if padded else None)
        if x.needs:
            dx, _ = gk.gconv(dy, u.wpt, u.cin, u.geom, out=grad_target(x), mode=gk.GATHER_DGRAD, out_hw=(x.t.shape[1], x.t.shape[2]))
            acc(x, dx, True)

    def conv_bias(self, x, u, out_f32=True):
        """nn.Conv2d with bias and no BatchNorm: the one-channel / class-logit heads in fp32 (agg1.conv5, PraNet_Res2Net.py:77; linear2..5,
        gcpa_cc2.py:37-40) or a bf16 feature conv (conv_d1 / conv_d2 / conv_l of FAM, gcpa_gald.py:66-74; the q / k / v projections of ccnet.py:43-51)."""
        if self.f32:
            return self.var(gk.gconv_f32(x.t, u.weight.detach(), u.geom, bias=u.bias.detach()), False)
        o, _ = _conv_forward(x.t, u, u.bias.detach(), False, out_f32=out_f32, net=self.net)

        def back(g):
            slot, accum = self.net._grad_slot(u.bias)
            gk.gbn_bwd_sums(g, None, None, None, None, slot, None, accumulate=accum)
            self._conv_backward(x, u, g if g.dtype == torch.bfloat16 else gk.gbinary(gk.OP_COPY, g, out_dtype=torch.bfloat16))
        return self.node(o, back)

    def binary(self, op, a, b, out=None):
        def back(g):
            if op == gk.OP_ADD:
                acc(a, g, False)
                acc(b, g, False)
            else:
                acc(a, gk.gbinary(gk.OP_MUL, g, b.t, out=grad_target(a)), True)
                acc(b, gk.gbinary(gk.OP_MUL, g, a.t, out=grad_target(b)), True)
        return self.node(gk.gbinary(op, a.t, b.t, out=out), back)

    def added(self, a, b, t):
        """The variable of t = a + b that a producer's apply has ALREADY written (conv_bn extras): binary(OP_ADD)'s place on the tape without its launch."""
        def back(g):
            acc(a, g, False)
            acc(b, g, False)
        return self.node(t, back)

    def alias_into(self, a, out):
        """copy_into whose copy the producer of `a` has already made (conv_bn extras)."""
        return self.node(out, lambda g: acc(a, g, False))

    def copy_into(self, a, out):
        return self.node(gk.gbinary(gk.OP_COPY, a.t, out=out), lambda g: acc(a, g, False))

    def avgpool(self, x, k, stride, pad, include_pad, out=None):
        H, W = x.t.shape[1], x.t.shape[2]
        if include_pad:
            Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        else:
            Ho, Wo = -(-H // stride), -(-W // stride)
        if self.f32:
            return self.var(gk.gpool_f32(x.t, k, stride, pad, 0 if include_pad else 1, (Ho, Wo), out=out), False)
        return self.node(gk.gavgpool(x.t, k, stride, pad, include_pad, (Ho, Wo), out=out),
                         lambda g: acc(x, gk.gavgpool_bwd(g, (H, W), k, stride, pad, include_pad, dx=grad_target(x)), True))

    def resize(self, x, factor, align, size=None):
        """F.interpolate(x, scale_factor=factor) or, with `size`, F.interpolate(x, size=size) (factor ignored), mode='bilinear'."""
        H, W = x.t.shape[1], x.t.shape[2]
        if size is not None:
            factor = None
        out_hw = tuple(size) if size is not None else (int(math.floor(H * factor)), int(math.floor(W * factor)))
        return self.node(gk.gresize(x.t, out_hw, align, factor), lambda g: acc(x, gk.gresize_bwd(g, (H, W), align, factor), True))

    def cat(self, buf, pieces):
        """`buf` already holds the pieces (their producers wrote into its channel slices); the gradient of the concatenation is handed to
        the pieces as slice views."""
        def back(g):
            off = 0
            for p in pieces:
                c = p.t.shape[-1]
                acc(p, g[..., off:off + c], True)
                off += c
        return self.node(buf, back)

    def split(self, parent, width, n):
        """torch.split as channel-slice views.  The slices' gradients are assembled side by side in one buffer that becomes the parent's
        gradient: `slots` (recorded by the caller AFTER the slices' consumers, so it runs before their backward) hands every slice its channel
        range; `gather` (recorded here, i.e. run after them) completes the buffer."""
        parts = [self.var(parent.t[..., i * width:(i + 1) * width]) for i in range(n)]
        state = {}

        def slots():
            B, H, W, C = parent.t.shape
            state["g"] = gk.new(B, H, W, C, parent.t.device)
            for i, p in enumerate(parts):
                p.want = state["g"][..., i * width:(i + 1) * width]

        def gather():
            for p in parts:
                if p.g is None:                                   # a slice nothing consumed
                    p.want.zero_()
                p.g = p.want = None
            acc(parent, state.pop("g"), True)
        self.record(gather)
        return parts, slots

    def backward(self):
        self.wq = _WgradQueue(WgradScheduler.on(self.net._store.data.device) if self.WGRAD_STREAM else WgradScheduler(None))
        for fn in reversed(self.tape):
            fn()
        self.tape = []
        self.wq.flush()
        self.wq.sched.join()          # the caller (optimizer, gradient exchange) sees complete weight gradients on its own stream
        self.wq = None


# ------------------------------------------------------------------------------------------------ the modules
class Engine(nn.Module):
    """Parameter storage and launch preparation shared by the modules of the tape nets: parameters registered under the reference's names,
    one flat fp32 buffer for them and one for their gradients (engine.FlatStore), every conv's bf16 operands packed by ONE table-driven
    launch when a weight changed, BatchNorm buffers as views of one buffer."""
    RUN = Run          # the tape class a module's graph is written against (host/pranet.py and host/gald.py extend it)
    SPARSE_OUTPUT_GRADS = False         # True: outputs without a gradient reach backward() as None instead of zero tensors (host/gald.py)

    def _register(self, order):
        """order: Unit objects and (key, tensor) pairs (parameters that belong to no conv: an unused classifier head, a scalar gate), in the
        reference's registration order (= state_dict order)."""
        self._units = []
        for u in order:
            if isinstance(u, tuple):
                key, value = u
                parent, leaf = key.rsplit(".", 1) if "." in key else ("", key)
                setattr(arch.node_at(self, parent) if parent else self, leaf, nn.Parameter(value))
                continue
            node = arch.node_at(self, u.key)
            kh, kw = u.geom[0], u.geom[1]
            w = torch.empty(u.cout, 1 if u.depthwise else u.cin, kh, kw)
            if u.key.startswith("resnet."):
                nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")          # Res2Net_v1b.py:113-115
            else:
                nn.init.kaiming_uniform_(w, a=math.sqrt(5))                              # nn.Conv2d default
            node.weight = nn.Parameter(w)
            u.weight = node.weight
            if u.bnkey is None or u.bias is True:      # a conv with bias (agg1.conv5; the FAM / local-attention convs in front of their BatchNorm)
                bound = 1.0 / math.sqrt((1 if u.depthwise else u.cin) * kh * kw)
                node.bias = nn.Parameter(torch.empty(u.cout).uniform_(-bound, bound))
                u.bias = node.bias
            if u.bnkey is not None:
                parent, leaf = u.bnkey.rsplit(".", 1) if "." in u.bnkey else ("", u.bnkey)
                (arch.node_at(self, parent) if parent else self).add_module(leaf, nn.BatchNorm2d(u.cout))
                u.bn = arch.node_at(self, u.bnkey)
            self._units.append(u)
        self._store = None
        self._pack_sig = None
        self._eval_cache = {}
        self._stat_flat = None
        self._stat_gen = 0
        self._ones_cache = {}

    def engine_parameters(self):
        return [(k, p) for k, p in self.named_parameters()]

    def ensure_flat(self):
        dev = self._units[0].weight.device
        if self._store is None or not self._store.intact() or self._store.data.device != dev:
            self._store = FlatStore(self.engine_parameters(), dev)
            self._pack_sig = None
            self._build_pack_plan(dev)
        if not self._buffers_intact(dev):
            self._flatten_buffers(dev)
        return self._store

    def _flatten_buffers(self, dev):
        """running_mean / running_var of every BatchNorm2d as views of one buffer, num_batches_tracked likewise: the counter of all the
        layers advances with ONE add per training forward."""
        bns = [u.bn for u in self._units if u.bn is not None]
        if not bns:                                          # a module without BatchNorm (CrissCrossAttention)
            self._stat_flat, self._nbt = torch.empty(0, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
            self._stat_gen += 1
            return
        n = sum(b.num_features for b in bns)
        flat = torch.empty(2 * n, dtype=torch.float32, device=dev)
        nbt = torch.empty(len(bns), dtype=torch.int64, device=dev)
        off = 0
        with torch.no_grad():
            for i, b in enumerate(bns):
                c = b.num_features
                for name, o in (("running_mean", off), ("running_var", n + off)):
                    v = flat[o:o + c]
                    v.copy_(getattr(b, name))
                    getattr(b, name).data = v          # keeps the buffer object (state_dict / load_state_dict see the view)
                nbt[i] = b.num_batches_tracked
                b.num_batches_tracked.data = nbt[i]
                off += c
        self._stat_flat, self._nbt = flat, nbt
        self._stat_gen += 1

    def _buffers_intact(self, dev):
        u = next((x for x in self._units if x.bn is not None), None)
        if u is None:
            return self._stat_flat is not None and self._stat_flat.device == dev
        return self._stat_flat is not None and self._stat_flat.device == dev and u.bn.running_mean.data_ptr() == self._stat_flat.data_ptr()

    def _build_pack_plan(self, dev):
        rows, off, blk = [], 0, 0
        packed = [u for u in self._units if not u.depthwise]          # depthwise kernels read the fp32 [C,1,3,3] weights directly
        for u in packed:
            kh, kw = u.geom[0], u.geom[1]
            n = gk.pack_elems(u.cout, u.cin, kh, kw)
            rows.append([u.weight._mi_off, off, off, u.cout, u.cin, kh * kw, blk, 0])
            blk += -(-n // 1024)
            off += n
        self._wp_flat = torch.empty(off, dtype=torch.bfloat16, device=dev)
        self._wpt_flat = torch.empty(off, dtype=torch.bfloat16, device=dev)
        for u, r in zip(packed, rows):
            n = gk.pack_elems(u.cout, u.cin, u.geom[0], u.geom[1])
            u.wp = self._wp_flat[r[1]:r[1] + n]
            u.wpt = self._wpt_flat[r[2]:r[2] + n]
        self._pack_blocks = blk
        self._pack_n = len(packed)
        self._pack_table = torch.tensor(rows, dtype=torch.int64, device=dev)

    def _prepare(self):
        st = self.ensure_flat()
        sig = (st.generation, sum(u.weight._version for u in self._units), st.data.data_ptr())
        if sig != self._pack_sig:
            if self._pack_n:                                 # (a module of depthwise convs only has nothing to pack: LocalAttenModule)
                gk.gconv_pack_multi(st.data, self._wp_flat, self._wpt_flat, self._pack_table, self._pack_n, self._pack_blocks)
            self._pack_sig = sig
        return st

    def _grad_slot(self, p):
        """(where d loss / d p is written, whether to accumulate: True from the second write of a backward pass on - shared parameters)."""
        st = self._store
        acc = id(p) in st.written
        st.written.add(id(p))
        g = st.grad[p._mi_off:p._mi_off + p.numel()].view_as(p)
        if p.grad is None or p.grad.data_ptr() != g.data_ptr():      # a zero_grad(set_to_none=True) dropped the view
            p.grad = g
        return g, acc

    def _grad_of(self, p):
        return self._grad_slot(p)[0]

    def zero_grad(self, set_to_none=True):
        """Gradient slots are overwritten by the next backward pass: forget which ones were written instead of clearing 100+ MB."""
        if self._store is not None:
            self._store.written.clear()
        else:
            super().zero_grad(set_to_none)

    def _ones(self, c):
        t = self._ones_cache.get(c)
        if t is None or t.device != self._store.data.device:
            t = self._ones_cache[c] = torch.ones(c, dtype=torch.float32, device=self._store.data.device)
        return t

    def _zeros(self, c):
        t = self._ones_cache.get(-c)
        if t is None or t.device != self._store.data.device:
            t = self._ones_cache[-c] = torch.zeros(c, dtype=torch.float32, device=self._store.data.device)
        return t

    def _eval_fold(self, u):
        bn = u.bn
        sig = (self._store.generation, self._stat_gen, bn.weight._version, bn.bias._version, bn.running_mean._version, bn.running_var._version)
        hit = self._eval_cache.get(u.key)
        if hit is None or hit[0] != sig:
            hit = (sig, gk.gbn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps))
            self._eval_cache[u.key] = hit
        return hit[1]

    precision = "bf16"

    def set_precision(self, precision):
        """'bf16': the training engine's regime in eval() too (bf16 activations and operands, fp32 accumulation).  'fp32': eval() forwards run in
        the reference's precision (csrc/gf32.hip) - what the testers use by default (TEST.PRECISION), so that the masks they threshold are the
        reference's.  train() forwards are bf16 either way."""
        if precision not in ("bf16", "fp32"):
            raise ValueError("precision must be 'bf16' or 'fp32', got %r" % (precision,))
        self.precision = precision
        return self

    def _graph(self, run, *inputs):
        raise NotImplementedError

    def _run(self, xs, rec, in_needs):
        for x in xs:
            if not x.is_cuda:
                raise _lib.MiError("%s runs on the MI355X only (got a %s tensor); the CPU restatement is oracle/ref_pranet.py, test infrastructure"
                                   % (type(self).__name__, x.device))
        self._prepare()
        run = self.RUN(self, self.training, rec)
        dt = torch.float32 if run.f32 else torch.bfloat16
        ins = [run.var(self._nhwc_input(x, dt, (need and rec) or not self.PAD_IMAGE), need) for x, need in zip(xs, in_needs)]      # NHWC bf16 (fp32 evaluation: fp32)
        outs = self._graph(run, *ins)
        if self.training:
            self._nbt.add_(1)
            self._stat_gen += 1                       # the kernels update the running statistics through raw pointers: no tensor version moves
        return run, ins, outs

    PAD_IMAGE = False          # True on the whole nets whose first op is the stem conv on the image (PraNet, GCPAEncoder)

    @staticmethod
    def _nhwc_input(x, dt, wants_grad):
        """NCHW module input -> NHWC activation.  A three-channel bf16 image that needs no gradient is stored with EIGHT channels (five zero planes): the stem
        conv then reads one 16-byte vector per pixel and tap instead of sixteen 2-byte loads (its packed weights are zero beyond channel 3 anyway), and its weight
        gradient is computed for eight input channels and cut back (see _conv_backward).  GALD's 3 -> 32 stem at 6 x 720 x 1280: 169 -> ~60 us forward, 320 -> ~100
        us weight gradient."""
        nhwc = x.detach().permute(0, 2, 3, 1)
        if dt == torch.bfloat16 and x.shape[1] == 3 and not wants_grad and os.environ.get("MI_STEM_PAD8", "1") != "0":
            out = torch.zeros((x.shape[0], x.shape[2], x.shape[3], 8), dtype=dt, device=x.device)
            out[..., :3] = nhwc
            return out
        return nhwc.to(dt).contiguous()

    def forward(self, *xs):
        self._grad_mode = torch.is_grad_enabled()          # (inside Function.forward grad mode is always off: ask here whether a tape is wanted at all)
        out = _EngineFn.apply(self, len(xs), *xs, *[p for _, p in self.engine_parameters()])
        return out[0] if len(out) == 1 else out


class _EngineFn(torch.autograd.Function):
    """An Engine module as one autograd node: forward records the tape, backward replays it; parameter gradients go straight into the
    flat gradient buffer that every `p.grad` is a view of (autograd receives None for them), input gradients are returned."""

    @staticmethod
    def forward(ctx, net, n_in, *args):
        xs = args[:n_in]
        in_needs = ctx.needs_input_grad[2:2 + n_in]
        rec = any(ctx.needs_input_grad[2:]) and getattr(net, "_grad_mode", True)
        run, ins, outs = net._run(xs, rec, in_needs)
        ctx.run, ctx.ins, ctx.outs, ctx.n_in, ctx.in_dtypes = run, ins, outs, n_in, [x.dtype for x in xs]
        if net.SPARSE_OUTPUT_GRADS:
            ctx.set_materialize_grads(False)          # an output no loss reached keeps no gradient (its producer's backward is skipped), not zeros
        return tuple(o.t.permute(0, 3, 1, 2) if o.t.dim() == 4 else o.t for o in outs)          # NCHW-shaped views of NHWC memory (or scalars: losses)

    @staticmethod
    def backward(ctx, *gouts):
        run = ctx.run
        for o, g in zip(ctx.outs, gouts):
            if g is not None:
                o.g, o.own = (g.permute(0, 2, 3, 1).to(o.t.dtype).contiguous() if g.dim() == 4 else g), True
        run.backward()
        run.net._store.zero_stale()          # parameters this pass did not reach must not keep the previous pass's gradient
        gin = [None if (v.g is None) else v.g.permute(0, 3, 1, 2).to(dt) for v, dt in zip(ctx.ins, ctx.in_dtypes)]
        ctx.run = ctx.ins = ctx.outs = None
        return (None, None) + tuple(gin) + (None,) * (len(ctx.needs_input_grad) - 2 - ctx.n_in)


# ------------------------------------------------------------------------------------------------ optimizer
class FlatAdam(torch.optim.Adam):
    """torch.optim.Adam(lr) over the module's flat parameter buffer with `clip_gradient(optimizer, clip)` (core/utils/utils.py:6-16) fused in:
    ONE launch per step (mi_adam_step_clamped) instead of one per tensor.  torch's state_dict format (per-parameter exp_avg / exp_avg_sq are
    views of the flat moment buffers).  Parameters the backward pass never writes (Res2Net's unused fc) keep a zero gradient: their moments
    stay zero and they do not move, like the reference's (whose fc.grad is None).

    `skip_unwritten` (opt-in, default False): a parameter that no backward pass wrote since zero_grad() is skipped entirely - its value,
    exp_avg, exp_avg_sq and its own `step` stay as they are, what torch.optim.Adam does for `p.grad is None`.  That matters once such a
    parameter has non-zero moments (GaldFada resumed from a GALD checkpoint: linear5/4/3 get no gradient there, and a zero-gradient update
    would keep moving them).  Steps are then counted per parameter (state_dict carries them); the written ones are updated with one launch
    per run of consecutive parameters that share a step count."""

    def __init__(self, net, lr, grad_clamp=None, skip_unwritten=False):
        self.net = net
        super().__init__(net.parameters(), lr)
        self.grad_clamp = grad_clamp
        self.skip_unwritten = skip_unwritten
        self._m = self._v = None
        self._steps = 0
        self._psteps = None              # {id(p): step} when the parameters' counts may differ (skip_unwritten, or loaded that way)
        self.device_hyper = None         # 6-float device tensor (lr, beta1, beta2, eps, clamp, step): HIP-graph mode

    def set_device_hyper(self, enable=True):
        """Graph mode: step() reads its hyper-parameters and the step count from device memory (mi_adam_step_dev); push_hyper() refreshes the
        learning rate from param_groups before a replay."""
        if not enable:
            self.device_hyper = None
            return
        self._ensure_moments()           # (allocated inside a capture they would be re-zeroed by every replay)
        g = self.param_groups[0]
        self.device_hyper = torch.tensor([g["lr"], g["betas"][0], g["betas"][1], g["eps"], self.grad_clamp or 0.0, float(self._steps)], dtype=torch.float32,
                                         device=self.net._store.data.device)

    def push_hyper(self):
        self.device_hyper[0:1].fill_(float(self.param_groups[0]["lr"]))

    def zero_grad(self, set_to_none=True):
        st = self.net._store
        if st is not None:
            st.written.clear()          # every gradient slot is overwritten by the next backward: no 130 MB memset

    def _ensure_moments(self):
        st = self.net.ensure_flat()
        if self._m is None or self._m.numel() != st.data.numel() or self._m.device != st.data.device:
            self._m, self._v = torch.zeros_like(st.data), torch.zeros_like(st.data)
            loaded = {}
            for p in st.params:
                s = self.state[p]
                if "exp_avg" in s:                                   # restored by load_state_dict: adopt
                    self._m[p._mi_off:p._mi_off + p.numel()].copy_(s["exp_avg"].reshape(-1))
                    self._v[p._mi_off:p._mi_off + p.numel()].copy_(s["exp_avg_sq"].reshape(-1))
                    loaded[id(p)] = int(s["step"])
                s["exp_avg"] = self._m[p._mi_off:p._mi_off + p.numel()].view_as(p)
                s["exp_avg_sq"] = self._v[p._mi_off:p._mi_off + p.numel()].view_as(p)
            if loaded:
                self._steps = max(loaded.values())
                if len(set(loaded.values())) > 1 or len(loaded) != len(st.params):
                    self._psteps = {id(p): loaded.get(id(p), 0) for p in st.params}
        return st

    @torch.no_grad()
    def step(self, closure=None):
        st = self._ensure_moments()
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("weight_decay", 0) != 0 or g.get("maximize"):
            raise NotImplementedError("FlatAdam implements the reference's configuration (pranet_trainer.py:20)")
        if self.skip_unwritten:
            return self._step_written(st, g)
        self._steps += 1
        self._psteps = None
        # a backward pass that never reached this module (detached features, a loss that bypasses it) ran no zero_stale(): the previous pass's gradients
        # would still sit in the flat buffer and be applied.  Cleared here: what torch's zero_grad(set_to_none=False) leaves (a no-op after a normal pass)
        st.zero_stale()
        if self.device_hyper is not None:
            if not torch.cuda.is_current_stream_capturing():
                self.push_hyper()
            self.device_hyper[5:6].add_(1.0)                           # (captured with the step: every replay advances the device-side count)
            K.adam_step_dev(st.data, st.grad, self._m, self._v, self.device_hyper)
        else:
            K.adam_step(st.data, st.grad, self._m, self._v, g["lr"], g["betas"][0], g["betas"][1], g["eps"], self._steps, grad_clamp=self.grad_clamp)
        st.generation += 1

    def _step_written(self, st, g):
        """skip_unwritten: Adam on the parameters the backward passes since zero_grad() wrote, each with its own step count."""
        if self.device_hyper is not None:
            raise NotImplementedError("FlatAdam: skip_unwritten has per-parameter step counts; the graph mode keeps one on the device")
        if self._psteps is None:
            self._psteps = {id(p): self._steps for p in st.params}
        self._steps += 1
        runs = []                                                       # [lo, hi, step]: consecutive written parameters, one step count
        for p in st.params:
            if id(p) not in st.written:
                runs.append(None)
                continue
            n = self._psteps[id(p)] = self._psteps[id(p)] + 1
            lo, hi = p._mi_off, p._mi_off + p.numel()
            if runs and runs[-1] is not None and runs[-1][2] == n:
                runs[-1][1] = hi                                        # (alignment gaps between them: zero gradient, zero moments, unchanged)
            else:
                runs.append([lo, hi, n])
        for r in runs:
            if r is not None:
                lo, hi, n = r
                K.adam_step(st.data[lo:hi], st.grad[lo:hi], self._m[lo:hi], self._v[lo:hi], g["lr"], g["betas"][0], g["betas"][1], g["eps"], n,
                            grad_clamp=self.grad_clamp)
        st.generation += 1

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._m = None                                                 # adopt the restored moments and step counts now
        self._ensure_moments()

    def state_dict(self):
        if self._psteps is not None:                                   # per-parameter counts
            for p in self.net._store.params:
                s = self.state[p]
                if "exp_avg" in s:
                    s["step"] = torch.tensor(float(self._psteps[id(p)]))
            return super().state_dict()
        step_t = torch.tensor(float(self._steps))                      # (graph replays advance the count without running step())
        for p, s in self.state.items():
            if "exp_avg" in s:
                s["step"] = step_t
        return super().state_dict()
