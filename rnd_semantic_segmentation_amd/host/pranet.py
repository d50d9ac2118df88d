"""The PraNet path on the MI355X engine (BASELINE config[3]): Res2Net-50 v1b (26w x 4s) trunk, three RFB blocks, the
partial decoder and three reverse-attention branches, forward AND backward as a schedule of C-ABI launches (csrc/gconv.hip, gnet.hip).

  PraNet            reference core/models/classifiers/pranet/PraNet_Res2Net.py:98-179 (same state_dict keys: 922, same four outputs)
  trunk             reference core/models/classifiers/pranet/Res2Net_v1b.py:15-170
  structure_loss    reference core/trainers/pranet_trainer.py:22-31
  PraNetTrainer     reference core/trainers/pranet_trainer.py:12-104
  PranetTester      reference core/testers/pranet_tester.py:10-53

The engine the graph below is written against (tape, modules as one autograd node, FlatAdam) and its design are in host/tape.py.
"""
import math
import os
from datetime import datetime

import torch

from .. import _lib
from .. import gk
from .. import kernels as K
from .plugin import BaseTrainer
from .tape import Engine, FlatAdam, Run, Unit, acc


class StructureLossFn(torch.autograd.Function):
    """loss = structure_loss(pred, mask) of pranet_trainer.py:22-31 (weighted IoU + the batch-mean BCE the reference's `reduce='none'`
    actually computes).  pred [B,1,H,W] fp32 (logits), mask [B,1,H,W] fp32 in [0,1]; the gradient flows to pred only."""

    @staticmethod
    def forward(ctx, pred, mask):
        loss, grad = K.structure_loss(pred.contiguous(), mask.contiguous(), want_grad=pred.requires_grad)
        ctx.save_for_backward(grad)
        return loss.clone()

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return (grad * gout if grad is not None else None), None


def structure_loss(pred, mask):
    return StructureLossFn.apply(pred.float(), mask.float())


# ------------------------------------------------------------------------------------------------ architecture table
def res2net_units(layers=(3, 4, 6, 3), base_width=26, scale=4):
    """Units of the Res2Net v1b trunk in the reference's registration order (= state_dict order), and a per-block description."""
    units = [Unit("resnet.conv1.0", "resnet.conv1.1", 3, 32, 3, 2, 1), Unit("resnet.conv1.3", "resnet.conv1.4", 32, 32, 3, 1, 1),
             Unit("resnet.conv1.6", "resnet.bn1", 32, 64, 3, 1, 1)]
    blocks = []
    inplanes = 64
    for li, (planes, n, stride) in enumerate(zip((64, 128, 256, 512), layers, (1, 2, 2, 2)), 1):
        width = int(math.floor(planes * (base_width / 64.0)))
        for b in range(n):
            name = "resnet.layer%d.%d" % (li, b)
            s = stride if b == 0 else 1
            blk = dict(name=name, width=width, stride=s, stage=b == 0, down=None)
            blk["conv1"] = Unit(name + ".conv1", name + ".bn1", inplanes, width * scale, 1)
            blk["convs"] = [Unit("%s.convs.%d" % (name, i), "%s.bns.%d" % (name, i), width, width, 3, s, 1) for i in range(scale - 1)]
            blk["conv3"] = Unit(name + ".conv3", name + ".bn3", width * scale, planes * 4, 1)
            order = [blk["conv1"]] + blk["convs"] + [blk["conv3"]]
            if b == 0 and (stride != 1 or inplanes != planes * 4):
                blk["down"] = Unit(name + ".downsample.1", name + ".downsample.2", inplanes, planes * 4, 1)
                order.append(blk["down"])
            units += order
            blocks.append(blk)
            inplanes = planes * 4
    return units, blocks


def _rfb_units(name, cin, c):
    u = {"b0": [Unit(name + ".branch0.0", None, cin, c, 1)]}
    for i, k in ((1, 3), (2, 5), (3, 7)):
        p = "%s.branch%d" % (name, i)
        u["b%d" % i] = [Unit(p + ".0", None, cin, c, 1), Unit(p + ".1", None, c, c, (1, k), 1, (0, k // 2)), Unit(p + ".2", None, c, c, (k, 1), 1, (k // 2, 0)),
                        Unit(p + ".3", None, c, c, 3, 1, k, k)]
    u["cat"] = Unit(name + ".conv_cat", None, 4 * c, c, 3, 1, 1)
    u["res"] = Unit(name + ".conv_res", None, cin, c, 1)
    flat = u["b0"] + u["b1"] + u["b2"] + u["b3"] + [u["cat"], u["res"]]
    for x in flat:                                   # BasicConv2d: <name>.conv.weight, <name>.bn.*
        x.bnkey = x.key + ".bn"
        x.key = x.key + ".conv"
    return u, flat


def _basic(name, cin, cout, k, pad=0):
    return Unit(name + ".conv", name + ".bn", cin, cout, k, 1, pad)


# ------------------------------------------------------------------------------------------------ PraNet's own tape ops
class _PraNetRun(Run):
    def stem_tail(self, x, u):
        """conv1.6 -> bn1 -> ReLU -> MaxPool2d(3, 2, 1) (Res2Net_v1b.py:149-152): conv with tile statistics, then normalise + ReLU + max-pool
        in ONE pass (mi_stem_pool_fwd with the batch affine); backward: pooled gradient routed by the stored argmax, then BatchNorm backward."""
        net, bn = self.net, u.bn
        if not self.train:
            sc, sh = net._eval_fold(u)
            if self.f32:
                return self.var(gk.gpool_f32(gk.gconv_f32(x.t, u.weight.detach(), u.geom, scale=sc, shift=sh, relu=True), 3, 2, 1, 2), False)
            y, _ = gk.gconv(x.t, u.wp, u.cout, u.geom)
            return self.var(K.stem_pool_fwd(y, sc, sh)[0], False)
        y, st = gk.gconv(x.t, u.wp, u.cout, u.geom, stats=True)
        M = y.shape[0] * y.shape[1] * y.shape[2]
        fin = gk.gbn_finalize(st, u.cout, M, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
        pool, idx = K.stem_pool_fwd(y, fin[2].contiguous(), fin[3].contiguous())

        def back(g):
            g = K.stem_pool_bwd(g.contiguous(), idx, net._ones(u.cout), (y.shape[1], y.shape[2]))      # d loss / d relu(bn(y)), already ReLU-masked
            dbeta, dgamma = net._grad_of(bn.bias), net._grad_of(bn.weight)
            gk.gbn_bwd_sums(g, y, None, fin[0], fin[1], dbeta, dgamma)
            dy = gk.gbn_bwd_apply(g, y, None, fin[0], fin[1], bn.weight, dbeta, dgamma, M)
            self._conv_backward(x, u, dy)
        return self.node(pool, back)

    def reverse_attention(self, gate, feat):
        if self.f32:
            return self.var(gk.gpoint_f32(gk.PW_REVERSE, feat.t, gate.t), False)

        def back(g):
            dfeat, dgate = gk.gra_bwd(gate.t, feat.t, g)
            acc(feat, dfeat, True)
            acc(gate, dgate, True)
        return self.node(gk.gra_fwd(gate.t, feat.t), back)

    def tversky_head(self, low, mask, alpha, eps, weights, phi=None, w_boundary=0.0):
        """CompoundLoss([TverskyLoss(alpha, eps), BinaryCrossEntropyLoss()], weights)(F.interpolate(low, size=mask.shape[-2:], mode="bilinear"), mask)
        (attn/loss.py on a side output of PraNet_Res2Net.py:127-170) fused, shaped like GALD's gdl_head: mi_upsample_tversky_bce never writes the
        full-resolution map, and its gradient pass has run by the time the loss exists (the coefficients stay on the device).  With phi (the signed
        distance map of the mask) the head adds w_boundary * mean(sigmoid(z) * phi) in the same launches (mi_upsample_tversky_bce_sdf)."""
        B, h, w, _ = low.t.shape
        extra = {} if phi is None else {"phi": phi, "w_boundary": w_boundary}
        loss_out, dlow, _ = K.upsample_tversky_bce(low.t.reshape(B, h, w), mask, want_grad=self.rec, alpha=alpha, eps=eps, weights=weights, align_corners=False,
                                                   **extra)
        return self.node(loss_out[0].clone(), lambda g: acc(low, dlow.view(B, h, w, 1) * g, True))


# ------------------------------------------------------------------------------------------------ graph pieces
def _bottle2neck(run, x, blk):
    """Res2Net_v1b.py:63-92: 1x1 to four `width`-channel groups; groups 0..2 through 3x3 convs, each (in a 'normal' block) taking the
    previous group's output added to its own input; group 3 passes through ('normal') or through AvgPool2d(3, stride, 1) ('stage')."""
    w, s, stage = blk["width"], blk["stride"], blk["stage"]
    B, H, W = x.t.shape[0], x.t.shape[1], x.t.shape[2]
    Ho, Wo = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    cat = gk.new(B, Ho, Wo, 4 * w, x.t.device, x.t.dtype)
    # 'normal' blocks (round 5): what used to be three element-wise launches comes out of the BatchNorm applies that produce the operands - conv1's apply also
    # writes the pass-through group into its slot of the concatenation, the apply of branch i also writes (its output + group i+1) = the next branch's input
    fuse = run.multi and not stage
    o1 = run.conv_bn(x, blk["conv1"], True, extras=[(3 * w, 4 * w, cat[..., 3 * w:], None)] if fuse else None)
    groups, slots = run.split(o1, w, 4)
    pieces, prev, sums, ahead = [], None, [], None
    for i in range(3):
        if i == 0 or stage:
            inp = groups[i]
        elif ahead is not None:
            inp = ahead
            sums.append((inp, groups[i]))
        else:
            inp = run.binary(gk.OP_ADD, prev, groups[i])
            sums.append((inp, groups[i]))
        nxt = gk.new(B, Ho, Wo, w, x.t.device, x.t.dtype) if (fuse and i < 2) else None
        prev = run.conv_bn(inp, blk["convs"][i], True, out=cat[..., i * w:(i + 1) * w], extras=None if nxt is None else [(0, w, nxt, groups[i + 1])])
        ahead = None if nxt is None else run.added(prev, groups[i + 1], nxt)
        pieces.append(prev)
    if stage:
        pieces.append(run.avgpool(groups[3], 3, s, 1, True, out=cat[..., 3 * w:]))
    else:
        pieces.append(run.alias_into(groups[3], cat[..., 3 * w:]) if fuse else run.copy_into(groups[3], cat[..., 3 * w:]))
    catv = run.cat(cat, pieces)
    if blk["down"] is not None:
        res = run.conv_bn(x if s == 1 else run.avgpool(x, s, s, 0, False), blk["down"], False)       # AvgPool2d(1, 1) is the identity
    else:
        res = x
    out = run.conv_bn(catv, blk["conv3"], True, add=res)

    def slots_and_sums():
        slots()
        for inp, grp in sums:          # the data gradient of convs[i] lands directly in group i's range: it IS d loss / d (prev + group i)
            inp.want = grp.want
    run.record(slots_and_sums)
    return out


def _rfb_block(run, x, units, c):
    """RFB_modified.forward (PraNet_Res2Net.py:50-59); BasicConv2d applies no ReLU (:17-20)."""
    B, H, W, _ = x.t.shape
    cat = gk.new(B, H, W, 4 * c, x.t.device, x.t.dtype)
    pieces = []
    for i in range(4):
        y = x
        chain = units["b%d" % i]
        for j, u in enumerate(chain):
            y = run.conv_bn(y, u, False, out=cat[..., i * c:(i + 1) * c] if j == len(chain) - 1 else None)
        pieces.append(y)
    xc = run.conv_bn(run.cat(cat, pieces), units["cat"], False)
    return run.conv_bn(x, units["res"], True, add=xc)                         # relu(x_cat + conv_res(x))


def _aggregation(run, a, c, x1, x2, x3):
    """aggregation.forward (PraNet_Res2Net.py:79-96); x1 coarsest."""
    up = lambda v: run.resize(v, 2, True)                                      # nn.Upsample(scale_factor=2, 'bilinear', align_corners=True)
    mul = lambda p, q, out=None: run.binary(gk.OP_MUL, p, q, out=out)
    B, H2, W2, _ = x2.t.shape
    _, H3, W3, _ = x3.t.shape
    cat2 = gk.new(B, H2, W2, 2 * c, x1.t.device, x1.t.dtype)
    cat3 = gk.new(B, H3, W3, 3 * c, x1.t.device, x1.t.dtype)
    up1 = up(x1)
    x2_1 = mul(run.conv_bn(up1, a["up1"], False), x2, out=cat2[..., :c])
    x3_1 = mul(mul(run.conv_bn(up(up1), a["up2"], False), run.conv_bn(up(x2), a["up3"], False)), x3, out=cat3[..., :c])
    p22 = run.conv_bn(up1, a["up4"], False, out=cat2[..., c:])
    x2_2 = run.conv_bn(run.cat(cat2, [x2_1, p22]), a["cat2"], False)
    p32 = run.conv_bn(up(x2_2), a["up5"], False, out=cat3[..., c:])
    x3_2 = run.conv_bn(run.cat(cat3, [x3_1, p32]), a["cat3"], False)
    return run.conv_bias(run.conv_bn(x3_2, a["conv4"], False), a["conv5"])


def _agg_units(prefix, c):
    a = prefix
    d = dict(up1=_basic(a + "conv_upsample1", c, c, 3, 1), up2=_basic(a + "conv_upsample2", c, c, 3, 1), up3=_basic(a + "conv_upsample3", c, c, 3, 1),
             up4=_basic(a + "conv_upsample4", c, c, 3, 1), up5=_basic(a + "conv_upsample5", 2 * c, 2 * c, 3, 1),
             cat2=_basic(a + "conv_concat2", 2 * c, 2 * c, 3, 1), cat3=_basic(a + "conv_concat3", 3 * c, 3 * c, 3, 1),
             conv4=_basic(a + "conv4", 3 * c, 3 * c, 3, 1), conv5=Unit(a + "conv5", None, 3 * c, 1, 1))
    return d, [d[k] for k in ("up1", "up2", "up3", "up4", "up5", "cat2", "cat3", "conv4", "conv5")]


def _reverse_branch(run, gate, feat, units):
    """One reverse-attention branch (PraNet_Res2Net.py:130-140 / :145-153 / :158-166): erase what the coarser map marks, predict a residual."""
    y = run.conv_bn(run.reverse_attention(gate, feat), units[0], False)
    for u in units[1:-1]:
        y = run.conv_bn(y, u, True)                                             # F.relu(self.raX_convY(x))
    r = run.conv_bn(y, units[-1], False, out_f32=True)
    return run.binary(gk.OP_ADD, r, gate)




# ------------------------------------------------------------------------------------------------ the modules
class Bottle2neck(Engine):
    """Res2Net_v1b.py:15-92 as a stand-alone module (same constructor arguments and state_dict keys); `downsample`: True builds the
    AvgPool2d(stride, stride, ceil_mode=True, count_include_pad=False) + 1x1 conv + BatchNorm2d path of Res2Net_v1b.py:120-127."""
    RUN = _PraNetRun
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, baseWidth=26, scale=4, stype="normal"):
        super().__init__()
        if scale != 4:
            raise NotImplementedError("the PraNet trunk is 26w x 4s")
        width = int(math.floor(planes * (baseWidth / 64.0)))
        blk = dict(name="", width=width, stride=stride, stage=stype == "stage", down=None)
        blk["conv1"] = Unit("conv1", "bn1", inplanes, width * scale, 1)
        blk["convs"] = [Unit("convs.%d" % i, "bns.%d" % i, width, width, 3, stride, 1) for i in range(scale - 1)]
        blk["conv3"] = Unit("conv3", "bn3", width * scale, planes * 4, 1)
        order = [blk["conv1"]] + blk["convs"] + [blk["conv3"]]
        if downsample:
            blk["down"] = Unit("downsample.1", "downsample.2", inplanes, planes * 4, 1)
            order.append(blk["down"])
        self._blk = blk
        self._register(order)

    def _graph(self, run, x):
        return [_bottle2neck(run, x, self._blk)]


class RFB_modified(Engine):
    """PraNet_Res2Net.py:22-59."""
    RUN = _PraNetRun

    def __init__(self, in_channel, out_channel):
        super().__init__()
        self._u, flat = _rfb_units("", in_channel, out_channel)
        for u in flat:
            u.key, u.bnkey = u.key.lstrip("."), u.bnkey.lstrip(".")
        self._c = out_channel
        self._register(flat)

    def _graph(self, run, x):
        return [_rfb_block(run, x, self._u, self._c)]


class aggregation(Engine):
    """PraNet_Res2Net.py:61-96: forward(x1, x2, x3), x1 coarsest; one-channel fp32 output."""
    RUN = _PraNetRun

    def __init__(self, channel):
        super().__init__()
        self._a, order = _agg_units("", channel)
        self._c = channel
        self._register(order)

    def _graph(self, run, x1, x2, x3):
        return [_aggregation(run, self._a, self._c, x1, x2, x3)]


class PraNet(Engine):
    """PraNet(channel=32) of PraNet_Res2Net.py:98-179.  forward(x [B,3,H,W]) -> (lateral_map_5, lateral_map_4, lateral_map_3, lateral_map_2),
    each [B,1,H,W] fp32 logits.  The reference loads ImageNet weights from a local file the image does not have; weights here are
    initialised like the reference's modules (kaiming_normal fan_out for the trunk's convs, Conv2d defaults elsewhere) or loaded from a
    checkpoint / the formula generator."""

    RUN = _PraNetRun
    PAD_IMAGE = True

    def __init__(self, channel=32):
        super().__init__()
        c = channel
        self.channel = c
        trunk, self._blocks = res2net_units()
        self._stem = trunk[:3]
        self._rfb = {}
        order = list(trunk)          # then Res2Net's classifier head: in the reference's state_dict, never run by PraNet
        order += [("resnet.fc.weight", torch.empty(1000, 2048).uniform_(-1, 1) / math.sqrt(2048)), ("resnet.fc.bias", torch.empty(1000).uniform_(-1, 1) / math.sqrt(2048))]
        for name, cin in (("rfb2_1", 512), ("rfb3_1", 1024), ("rfb4_1", 2048)):
            self._rfb[name], flat = _rfb_units(name, cin, c)
            order += flat
        self._agg, agg_order = _agg_units("agg1.", c)
        order += agg_order
        self._ra = {4: [_basic("ra4_conv1", 2048, 256, 1)] + [_basic("ra4_conv%d" % i, 256, 256, 5, 2) for i in (2, 3, 4)] + [_basic("ra4_conv5", 256, 1, 1)],
                    3: [_basic("ra3_conv1", 1024, 64, 1), _basic("ra3_conv2", 64, 64, 3, 1), _basic("ra3_conv3", 64, 64, 3, 1), _basic("ra3_conv4", 64, 1, 3, 1)],
                    2: [_basic("ra2_conv1", 512, 64, 1), _basic("ra2_conv2", 64, 64, 3, 1), _basic("ra2_conv3", 64, 64, 3, 1), _basic("ra2_conv4", 64, 1, 3, 1)]}
        order += self._ra[4] + self._ra[3] + self._ra[2]
        self._register(order)

    def _graph(self, run, x):
        if x.t.shape[1] % 32 or x.t.shape[2] % 32:
            raise _lib.MiError("PraNet input sides must be multiples of 32 (the reverse-attention branches resize by exact factors), got %s" % (tuple(x.t.shape),))
        s = self._stem
        y = run.tap("stem0", run.conv_bn(x, s[0], True))
        y = run.tap("stem1", run.conv_bn(y, s[1], True))
        y = run.tap("stem", run.stem_tail(y, s[2]))
        ends = {}
        for blk in self._blocks:
            y = run.tap(blk["name"], _bottle2neck(run, y, blk))
            ends[blk["name"].rsplit(".", 1)[0]] = y                                  # the last block of each layer wins
        x2, x3, x4 = ends["resnet.layer2"], ends["resnet.layer3"], ends["resnet.layer4"]
        x2r = _rfb_block(run, x2, self._rfb["rfb2_1"], self.channel)
        x3r = _rfb_block(run, x3, self._rfb["rfb3_1"], self.channel)
        x4r = _rfb_block(run, x4, self._rfb["rfb4_1"], self.channel)
        run.tap("rfb2", x2r), run.tap("rfb3", x3r), run.tap("rfb4", x4r)
        coarse = run.tap("coarse", _aggregation(run, self._agg, self.channel, x4r, x3r, x2r))           # ra5_feat: 1/8 resolution, one channel, fp32
        rs = lambda v, f: run.resize(v, f, False)                                    # F.interpolate(..., mode='bilinear'): align_corners False
        tv = self.__dict__.get("_tversky")
        head = rs if tv is None else (lambda v, f: run.tversky_head(v, *tv))          # losses(): the map's last resize and its loss in one kernel
        maps = [head(coarse, 8)]
        g = run.tap("ra4", _reverse_branch(run, rs(coarse, 0.25), x4, self._ra[4]))
        maps.append(head(g, 32))
        g = run.tap("ra3", _reverse_branch(run, rs(g, 2), x3, self._ra[3]))
        maps.append(head(g, 16))
        g = run.tap("ra2", _reverse_branch(run, rs(g, 2), x2, self._ra[2]))
        maps.append(head(g, 8))
        if tv is not None:
            return maps                                                              # four scalar losses
        return [run.tap("map%d" % i, m) for i, m in enumerate(maps)]

    def losses(self, x, gts, alpha=0.7, eps=1.0, weights=(0.5, 0.5), boundary_weight=0.0):
        """(loss5, loss4, loss3, loss2) = CompoundLoss([TverskyLoss(alpha, eps), BinaryCrossEntropyLoss()], weights)(lateral_map_i, gts) (attn/loss.py)
        without materialising the four [B,1,H,W] maps: each head's final upsample, its loss and the gradient are one fused call on the low-resolution
        map (mi_upsample_tversky_bce).  gts [B,1,H,W] or [B,H,W], values in [0, 1], the size of x.
        boundary_weight > 0 adds that many times the boundary loss mean(sigmoid(z) * phi) to every head: phi, the signed distance map of (gts >= 0.5), is
        computed once on the device (mi_signed_distance) and shared by the four heads; at 0 neither it nor the heads' phi mode is launched."""
        if not 0.0 <= float(alpha) <= 1.0 or not float(eps) > 0.0 or len(weights) != 2:
            raise ValueError("PraNet.losses: alpha in [0, 1], eps > 0 and weights = (tversky, bce), got %r / %r / %r" % (alpha, eps, weights))
        if gts.dim() not in (3, 4) or (gts.dim() == 4 and gts.shape[1] != 1) or (gts.shape[0], gts.shape[-2], gts.shape[-1]) != (x.shape[0], x.shape[2], x.shape[3]):
            raise ValueError("PraNet.losses: gts must be [B,1,H,W] or [B,H,W] of the images' size %s, got %s" % (tuple(x.shape), tuple(gts.shape)))
        boundary_weight = _boundary_weight(boundary_weight, "PraNet.losses")
        mask = gts.detach().float().reshape(gts.shape[0], gts.shape[-2], gts.shape[-1]).contiguous()
        self._tversky = (mask, float(alpha), float(eps), (float(weights[0]), float(weights[1])))
        if boundary_weight > 0.0:
            self._tversky += (K.signed_distance(mask, 0.5), boundary_weight)
        try:
            return super().forward(x)
        finally:
            self._tversky = None


# ------------------------------------------------------------------------------------------------ schedule / trainer / tester
def _boundary_weight(weight, who):
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= weight < float("inf"):          # (a nan fails both comparisons)
        raise ValueError("%s: boundary_weight must be a finite number >= 0, got %r" % (who, weight))
    return float(weight)


def step_losses(net, images, gts, criterion="ce", alpha=0.7, literal=False, boundary_weight=0.0):
    """The four losses (lateral 5, 4, 3, 2) of one step.  "ce": the trainer's own structure loss on the four maps (pranet_trainer.py:50-54);
    "tversky": CompoundLoss([TverskyLoss(alpha), BinaryCrossEntropyLoss()]) per side output, the terms MultiscaleLoss adds up (attn/loss.py; every
    head's label is `gts`) - fused with the heads' upsamples (PraNet.losses), or with literal=True (tests and tools/pranet_bench.py only) the
    composition without the fusion: net(images) materialises the four maps, each goes through the host/losses.py modules.
    boundary_weight > 0 ("tversky" only): plus that many times the boundary loss per side output - inside the fused heads, or with literal=True as a
    third term BoundaryLoss() of the compound."""
    boundary_weight = _boundary_weight(boundary_weight, "step_losses")
    if boundary_weight > 0.0 and criterion == "ce":
        raise ValueError("step_losses: boundary_weight needs criterion 'tversky' (the structure loss has no boundary term)")
    if criterion == "ce":
        return [structure_loss(o, gts) for o in net(images)]
    if criterion != "tversky":
        raise ValueError("criterion must be 'ce' or 'tversky', got %r" % (criterion,))
    if literal:
        from .losses import BinaryCrossEntropyLoss, BoundaryLoss, CompoundLoss, TverskyLoss
        crit = CompoundLoss([TverskyLoss(alpha=alpha), BinaryCrossEntropyLoss()])
        if boundary_weight > 0.0:
            crit = CompoundLoss([TverskyLoss(alpha=alpha), BinaryCrossEntropyLoss(), BoundaryLoss()], weights=[0.5, 0.5, boundary_weight])
        return [crit(o, gts) for o in net(images)]
    if boundary_weight > 0.0:
        return list(net.losses(images, gts, alpha=alpha, boundary_weight=boundary_weight))
    return list(net.losses(images, gts, alpha=alpha))


class GraphedStep:
    """One whole optimizer step of pranet_trainer.py:39-60 - weight pack, forward, four losses (step_losses), backward, clamped Adam: ~1 800
    launches - captured once as a HIP graph and replayed: the host cost of a step becomes one graph launch.  Inputs are copied into static
    buffers; the learning rate and Adam's step count live in device memory (FlatAdam.set_device_hyper)."""

    def __init__(self, net, opt, images, gts, warmup=3, criterion="ce", alpha=0.7, literal=False, boundary_weight=0.0):
        self.net, self.opt = net, opt
        self.criterion, self.alpha, self.literal, self.boundary_weight = criterion, alpha, literal, boundary_weight
        self.x, self.gt = images.detach().clone(), gts.detach().clone()
        net.ensure_flat()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                  # eager warm-up on the capture stream's pool: workspaces, moment buffers, caches
            for _ in range(warmup):
                self._core()
        torch.cuda.current_stream().wait_stream(side)
        opt.set_device_hyper(True)
        torch.cuda.synchronize()
        net._pack_sig = None                           # the weight pack belongs inside the graph: weights change on every replay
        steps = opt._steps
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.losses = self._core()
        opt._steps = steps                             # the capture itself executed nothing

    def _core(self):
        self.opt.zero_grad()
        ls = step_losses(self.net, self.x, self.gt, self.criterion, self.alpha, self.literal, self.boundary_weight)
        (ls[3] + ls[2] + ls[1] + ls[0]).backward()
        self.opt.step()
        return [l.detach() for l in ls]

    def __call__(self, images=None, gts=None):
        """Returns the four losses (lateral 5, 4, 3, 2) as device scalars owned by the graph (clone to keep across replays)."""
        if images is not None:
            self.x.copy_(images, non_blocking=True)
            self.gt.copy_(gts, non_blocking=True)
        self.opt.push_hyper()
        self.graph.replay()
        self.opt._steps += 1
        self.net._stat_gen += 1
        self.net._store.generation += 1
        return self.losses


def graph_mode_default():
    """PraNetTrainer replays its optimizer step as a HIP graph unless MI_GRAPH=0: ~1 300 launches of 3 - 40 us per step leave the host 15 - 20 % behind the
    GPU when enqueued one by one (bench.py prints both numbers); the replay is bit-equal to eager (tests/test_gpu_pranet.py)."""
    return os.environ.get("MI_GRAPH", "1") != "0"


def warmup_cosine_lr(base_lr, steps, multiplier=8.0, warm=5, t_max=100):
    """Learning rate after `steps` calls of scheduler.step() in pranet_trainer.py:97-104: GradualWarmupScheduler(multiplier=8, total_epoch=5)
    (core/utils/adapt_lr.py:19-45) climbs linearly from base_lr to 8 * base_lr over 5 epochs, then hands over to CosineAnnealingLR(T_max=100,
    eta_min=0).  The hand-over as the reference's chain performs it (pinned by tests/golden/g12_pranet_lr.npz, written by running that chain):
    the cosine scheduler continues RECURSIVELY from the group's current rate 8 * base_lr with its own epoch counter already at 1, so epoch
    warm + 1 overshoots to 8 * base_lr * 2 / (1 + cos(pi / t_max)) and every later rate keeps that factor over the textbook closed form."""
    if steps <= warm:
        return base_lr * ((multiplier - 1.0) * steps / warm + 1.0)
    t = steps - warm - 1
    return base_lr * multiplier * (1.0 + math.cos(math.pi * t / t_max)) / (1.0 + math.cos(math.pi / t_max))


def clip_gradient(optimizer, grad_clip):
    """core/utils/utils.py:6-16 (API parity; PraNetTrainer fuses the clamp into FlatAdam's update instead)."""
    for group in optimizer.param_groups:
        for param in group["params"]:
            if param.grad is not None:
                param.grad.data.clamp_(-grad_clip, grad_clip)


class AvgMeter:
    """core/utils/utils.py:18-38."""

    def __init__(self, num=40):
        self.num = num
        self.losses = []

    def update(self, val, n=1):
        self.losses.append(val)

    def show(self):
        return torch.mean(torch.stack(self.losses[max(len(self.losses) - self.num, 0):]))


class PraNetTrainer(BaseTrainer):
    """pranet_trainer.py:12-104: Adam(BASE_LR / 8), three passes per batch (the reference's multi-scale loop, whose rescale is a no-op:
    it resizes to trainsize whatever the rate - Appendix B), structure loss on the four side outputs, gradient clamp 0.5, warm-up + cosine
    schedule per epoch, checkpoint {'epoch', 'model', 'optimizer'} as PraNet-<epoch>.pth.  SOLVER.LOSS "ce" (default) is that structure loss;
    "tversky" replaces it with the Tversky + BCE compound of attn/loss.py on the same four outputs (step_losses), everything else unchanged;
    SOLVER.BOUNDARY_WEIGHT > 0 adds the boundary loss on the label's signed distance map to each of those four heads."""

    LOSSES = ("ce", "tversky")

    def __init__(self, name, cfg, train_loader, local_rank, logger=None):
        super().__init__(name, cfg, train_loader, local_rank, logger)

    def init_params(self):
        self.loss_name = getattr(self.cfg.SOLVER, "LOSS", "ce")                  # (not in the reference's config: host/config.py)
        self.tversky_alpha = float(getattr(self.cfg.SOLVER, "TVERSKY_ALPHA", 0.7))
        self.boundary_weight = float(getattr(self.cfg.SOLVER, "BOUNDARY_WEIGHT", 0.0))      # > 0: "tversky" only (plugin.require_loss refused the rest)
        self.trainsize = self.cfg.INPUT.TRAINSIZE
        self.model = PraNet().to(self.device)
        self.model.ensure_flat()
        self.base_lr = self.cfg.SOLVER.BASE_LR / 8
        self.optimizer = FlatAdam(self.model, self.base_lr, grad_clamp=0.5)

    structure_loss = staticmethod(structure_loss)

    def _resize_to_trainsize(self, t):
        """F.upsample(t, size=(trainsize, trainsize), mode='bilinear', align_corners=True) of pranet_trainer.py:47-48."""
        if t.shape[-2:] == (self.trainsize, self.trainsize):
            return t                                               # same size with align_corners=True: the identity
        nhwc = t.float().permute(0, 2, 3, 1).contiguous()
        return gk.gresize(nhwc, (self.trainsize, self.trainsize), True).permute(0, 3, 1, 2).contiguous()

    GRAPH_WARMUP = 3

    def train_step(self, images, gts):
        """One optimizer step (pranet_trainer.py:39-60).  Returns the four losses (lateral 5, 4, 3, 2) as device scalars.
        After three eager steps the step is captured as a HIP graph and replayed while the input shape stays the same (MI_GRAPH=0: always eager)."""
        if graph_mode_default():
            st = self.__dict__.setdefault("_graph", {"eager": 0, "step": None, "shape": None})
            if st["step"] is not None and st["shape"] == (tuple(images.shape), tuple(gts.shape)):
                return [l.clone() for l in st["step"](images, gts)]
            if st["step"] is None and st["eager"] >= self.GRAPH_WARMUP:
                st["step"] = GraphedStep(self.model, self.optimizer, images, gts, warmup=0, criterion=self.loss_name, alpha=self.tversky_alpha,
                                         boundary_weight=self.boundary_weight)
                st["shape"] = (tuple(images.shape), tuple(gts.shape))
                return [l.clone() for l in st["step"](images, gts)]
            st["eager"] += 1
        self.optimizer.zero_grad()
        if self.loss_name == "ce":
            outs = self.model(images)
            losses = [self.structure_loss(o, gts) for o in outs]
        else:
            losses = step_losses(self.model, images, gts, self.loss_name, self.tversky_alpha, boundary_weight=self.boundary_weight)
        loss = losses[3] + losses[2] + losses[1] + losses[0]
        loss.backward()
        self.optimizer.step()                                       # clip_gradient(optimizer, 0.5) is fused into the update
        return losses

    def _train_epoch(self, epoch):
        size_rates = [0.75, 1, 1.25]
        rec = [AvgMeter() for _ in range(4)]                        # lateral 2, 3, 4, 5
        n = len(self.train_loader)
        for i, pack in enumerate(self.train_loader):
            for rate in size_rates:
                images, gts, _ = pack
                images = images.to(self.device, non_blocking=True)
                gts = gts.to(self.device, non_blocking=True).float()
                if gts.dim() == 3:
                    gts = gts.unsqueeze(1)
                if rate != 1:
                    images, gts = self._resize_to_trainsize(images), self._resize_to_trainsize(gts)
                l5, l4, l3, l2 = self.train_step(images, gts)
                if rate == 1:
                    for m, v in zip(rec, (l2, l3, l4, l5)):
                        m.update(v.detach(), self.cfg.SOLVER.BATCH_SIZE)
            if i % 20 == 0 or i == n:
                self.logger.info("{} Epoch [{:03d}/{:03d}], Step [{:04d}/{:04d}], [lateral-2: {:.4f}, lateral-3: {:0.4f}, lateral-4: {:0.4f}, lateral-5: {:0.4f}, "
                                 "learning_rate: {:0.8f}]".format(datetime.now(), epoch, self.cfg.SOLVER.EPOCHS, i, n, rec[0].show(), rec[1].show(), rec[2].show(),
                                                                  rec[3].show(), self.optimizer.param_groups[0]["lr"]))
        save_path = self.cfg.OUTPUT_DIR
        os.makedirs(save_path, exist_ok=True)
        if epoch % self.cfg.SOLVER.CHECKPOINT_PERIOD == 0:
            self._save_checkpoint(epoch, save_path + "PraNet-%d.pth" % epoch)
            self.logger.info("[Saving Snapshot:] " + save_path + "PraNet-{}.pth".format(epoch))

    def _val_epoch(self, epoch):
        raise NotImplementedError("the reference's PraNetTrainer has no validation epoch")

    def _save_checkpoint(self, epoch, save_path):
        torch.save({"epoch": epoch, "model": self.model.state_dict(), "optimizer": self.optimizer.state_dict()}, save_path)

    def _load_checkpoint(self):
        self.checkpoint = torch.load(self.cfg.resume, map_location=self.device)
        self.model.load_state_dict(self.checkpoint["model"])
        if "optimizer" in self.checkpoint:
            self.logger.info("Loading optimizer from {}".format(self.cfg.resume))
            self.optimizer.load_state_dict(self.checkpoint["optimizer"])
        if "epoch" in self.checkpoint:
            self.start_epoch = self.checkpoint["epoch"] + 1

    def train(self):
        self.model.train()
        self.logger.info("#" * 20 + " Start Training " + "#" * 20)
        for k, epoch in enumerate(range(self.start_epoch, self.cfg.SOLVER.EPOCHS + 1)):
            for grp in self.optimizer.param_groups:                   # the reference builds fresh schedulers per run: k steps since start
                grp["lr"] = warmup_cosine_lr(self.base_lr, k)
            self._train_epoch(epoch)


class PranetTester:
    """pranet_tester.py:10-53: res2 -> resize to the label size (align_corners False) -> sigmoid -> min-max normalise over the batch ->
    {background, polyp} by which of (1 - p, p) is larger -> intersection / union meters.  TEST.POLYP_METRICS True (not in the reference) adds
    the polyp-segmentation metrics - mean Dice / IoU, F-beta, S-measure, E-measure, MAE - from one fused tail (score) and writes
    OUTPUT_DIR/pranet_polyp_metrics.json; the intersection / union meters are then fed from that tail's mask.  TEST.SURFACE_METRICS True (not
    in the reference either) measures the same mask against the label with kernels.surface_score - Hausdorff distance, its percentile, average
    symmetric surface distance, surface Dice - and writes OUTPUT_DIR/pranet_surface_metrics.json; the other outputs do not change.
    TEST.LESION_METRICS True (not in the reference) counts lesion-wise detections on the connected components of that mask and of the label with
    kernels.lesion_score and writes OUTPUT_DIR/pranet_lesion_metrics.json.  TEST.MASK_MIN_AREA / TEST.MASK_KEEP_LARGEST filter the mask's
    components in the same call: the filtered mask then replaces the mask for the intersection / union meters, the surface metrics and the lesion
    counts.  The polyp metrics are measured on the soft map and are NOT filtered."""

    def __init__(self, cfg, device, test_loader, logger):
        from .metrics import (lesion_settings, polyp_settings, require_no_boundary, require_no_crf, require_no_curves, require_no_slide,
                              require_plain_argmax, require_single_scale, surface_settings)
        require_single_scale(cfg, "PranetTester")
        require_plain_argmax(cfg, "PranetTester")
        require_no_crf(cfg, "PranetTester")
        require_no_slide(cfg, "PranetTester")
        require_no_boundary(cfg, "PranetTester")
        require_no_curves(cfg, "PranetTester")
        self.cfg, self.logger, self.test_loader, self.device = cfg, logger, test_loader, device
        self.polyp_metrics = polyp_settings(cfg)                      # TEST.POLYP_METRICS: test() scores through kernels.polyp_score
        self.surface = surface_settings(cfg)                          # TEST.SURFACE_METRICS: None, or (percentile, tolerances) for kernels.surface_score
        self.lesion = lesion_settings(cfg)                            # TEST.LESION_METRICS / MASK_*: None, or (metrics, connectivity, overlap, min_area, keep_largest)
        self.model = PraNet()
        self.model.to(device)
        # The reference thresholds an fp32 forward (pranet_tester.py:36-46): TEST.PRECISION 'fp32' (default) evaluates in the reference's precision
        # (csrc/gf32.hip: maps within 1e-5 of the reference's, masks identical), 'bf16' in the training engine's regime (faster).
        self.model.set_precision(cfg.TEST.PRECISION if "PRECISION" in cfg.TEST else "fp32")

    def _load_checkpoint(self):
        self.logger.info("Loading checkpoint from {}".format(self.cfg.resume))
        checkpoint = torch.load(self.cfg.resume, map_location=self.device)
        self.model.load_state_dict(checkpoint["model"])

    def predict(self, x, hw):
        with torch.no_grad():
            res2 = self.model(x)[3].float()
            out = gk.gresize(res2.permute(0, 2, 3, 1).contiguous(), hw, False).permute(0, 3, 1, 2)
            p = out.sigmoid().squeeze(1)
            p = (p - p.min()) / (p.max() - p.min() + 1e-8)
            return (p > 1 - p).long()                                  # np.stack([1 - p, p]).max(1)[1]: ties go to background

    def score(self, x, y, names=None):
        """TEST.POLYP_METRICS: one batch through the fused tail (kernels.polyp_score: resize, sigmoid, batch min-max, histogram, moment sums and
        the mask of predict in four small launches).  Returns (pred int64 [B,H,W], [polyp_image_stats per image]); a label outside {0, 1} raises
        ValueError naming the image - the S-measure's geometry has no meaning with holes."""
        from .. import kernels
        from .metrics import polyp_image_stats
        with torch.no_grad():
            res2 = self.model(x)[3].float()
        r = kernels.polyp_score(res2.reshape(res2.shape[0], res2.shape[2], res2.shape[3]).contiguous(), y.contiguous(), want_prob=False, want_pred=True)
        hist, sums, counts = r.hist.cpu().numpy(), r.sums.cpu().numpy(), r.counts.cpu().numpy()
        for b in range(y.shape[0]):
            if counts[b, 3]:
                name = names[b] if names is not None and len(names) > b else "#%d of the batch" % b
                raise ValueError("PranetTester: TEST.POLYP_METRICS needs labels in {0, 1}; image %s has %d others" % (name, int(counts[b, 3])))
        self.last_mask = r.pred                                       # the tail's uint8 mask, for surface()
        return r.pred.long(), [polyp_image_stats(hist[b], sums[b], y.shape[1], y.shape[2]) for b in range(y.shape[0])]

    def surface_stats(self, mask, y):
        """TEST.SURFACE_METRICS: one batch's mask (uint8 [B,H,W]) and labels through kernels.surface_score (foreground = 1, every other label is
        background); one small copy to the host.  Returns [surface_image_stats per image]."""
        from .. import kernels
        from .metrics import surface_image_stats
        percentile, tolerances = self.surface
        r = kernels.surface_score(mask.contiguous(), y.contiguous(), 1, percentile, tolerances)
        ints, sums = r.ints.cpu().numpy(), r.sums.cpu().numpy()
        return [surface_image_stats(ints[b], sums[b], tolerances, percentile) for b in range(y.shape[0])]

    def lesion_stats(self, mask, y):
        """TEST.LESION_METRICS / TEST.MASK_MIN_AREA / TEST.MASK_KEEP_LARGEST: one batch's mask (uint8 [B,H,W]) and labels through
        kernels.lesion_score (foreground = 1, every other label is background); one small copy to the host.  Returns (the filtered mask uint8
        [B,H,W] on the device, [lesion_image_stats per image])."""
        from .. import kernels
        from .metrics import lesion_image_stats
        _, connectivity, overlap, min_area, keep_largest = self.lesion
        r = kernels.lesion_score(mask.contiguous(), y.contiguous(), 1, connectivity, min_area, keep_largest, overlap)
        ints = r.ints.cpu().numpy()
        return r.filtered, [lesion_image_stats(ints[b]) for b in range(y.shape[0])]

    def test(self):
        from .metrics import AverageMeter, LesionMeter, PolypMeter, SurfaceMeter, dump_json, intersectionAndUnionGPU
        self.model.eval()
        self.meter = AverageMeter()
        self.polyp_meter = PolypMeter() if self.polyp_metrics else None
        self.surface_meter = SurfaceMeter(*self.surface) if self.surface is not None else None
        self.lesion_meter = LesionMeter() if self.lesion is not None and self.lesion[0] else None
        mask_filter = self.lesion is not None and (self.lesion[3] > 0 or self.lesion[4])
        for x, y, names in self.test_loader:
            x = x.to(self.device, non_blocking=True)
            y = y.to(self.device, non_blocking=True)
            h, w = y.shape[-2:]
            y = y.reshape(y.shape[0], h, w).long()
            if self.polyp_metrics:
                pred, stats = self.score(x, y, names)
                for s in stats:
                    self.polyp_meter.update(s)
            else:
                pred = self.predict(x, (h, w))
            mask = self.last_mask if self.polyp_metrics else None    # the uint8 mask the surface and lesion kernels read
            if self.lesion is not None:
                filtered, stats = self.lesion_stats(mask if mask is not None else pred.to(torch.uint8), y)
                if self.lesion_meter is not None:
                    for s in stats:
                        self.lesion_meter.update(s)
                if mask_filter:                                        # from here on the filtered mask is the prediction
                    mask, pred = filtered, filtered.long()
            if self.surface is not None:
                for s in self.surface_stats(mask if mask is not None else pred.to(torch.uint8), y):
                    self.surface_meter.update(s)
            inter, union, target, res = intersectionAndUnionGPU(pred, y, self.cfg.MODEL.NUM_CLASSES, self.cfg.INPUT.IGNORE_LABEL)
            self.meter.update(inter.cpu().numpy(), union.cpu().numpy(), target.cpu().numpy(), res.cpu().numpy())
        self.meter.summary(self.logger, self.cfg.MODEL.NUM_CLASSES)
        if self.polyp_metrics:
            self.polyp_meter.summary(self.logger)
            os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
            curves = self.polyp_meter.mean_curves()
            dump_json(os.path.join(self.cfg.OUTPUT_DIR, "pranet_polyp_metrics.json"),
                      dict(self.polyp_meter.as_dict(), dice_curve=curves["dice"].tolist(), iou_curve=curves["iou"].tolist()))
        if self.surface is not None:
            self.surface_meter.summary(self.logger)
            os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
            dump_json(os.path.join(self.cfg.OUTPUT_DIR, "pranet_surface_metrics.json"),
                      dict(self.surface_meter.as_dict(), percentile=self.surface[0], tolerances=list(self.surface[1])))
        if mask_filter:
            self.logger.info("Mask filter: components below {} pixels removed{} (connectivity {}) before the intersection / union{} lines; "
                             "the polyp metrics are not filtered.".format(self.lesion[3], ", only the largest kept" if self.lesion[4] else "",
                                                                          self.lesion[1], " and surface" if self.surface is not None else ""))
        if self.lesion_meter is not None:
            self.lesion_meter.summary(self.logger)
            os.makedirs(self.cfg.OUTPUT_DIR, exist_ok=True)
            dump_json(os.path.join(self.cfg.OUTPUT_DIR, "pranet_lesion_metrics.json"),
                      dict(self.lesion_meter.as_dict(), connectivity=self.lesion[1], overlap=self.lesion[2], min_area=self.lesion[3],
                           keep_largest=self.lesion[4]))
