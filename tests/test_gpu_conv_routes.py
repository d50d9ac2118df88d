"""Float64 parity of every implicit-GEMM conv route the DeepLab bench workloads launch (tests/_conv_cases.py: PRODUCTION, CASES).

Each case runs at default switches, at a shape for which the dispatcher picks the route the case names (asserted through kernels.ROUTES), against float64 torch
(F.conv2d and its autograd, on the device) on the same bf16-rounded operands, with the epilogue of the route computed in float64 in the kernel's order (scale and
shift, residual, ReLU / LeakyReLU, mask):
  - bf16 outputs within _parity._close_bf16 (1 ulp of the element + 2e-5 of the max: fp32 accumulation, one rounding), fp32 outputs (OUT_F32, the ZSPLIT tap
    planes) within 2e-5 of the max;
  - mask_out bits equal to (stored output > 0) on every element; outputs under a cleared bit of a ReLU-backward mask exactly zero;
  - the statistics epilogue: per partial row tile (h = 16 * MT rows of one wave row; 16 * MTG for the ping-pong loop) and channel, the kernel adds
    d = fl(o - pilot) of the bf16-ROUNDED outputs o, and d * d, in fp32.  Any summation tree over h terms puts at most h - 1 additions on a term, so with
    u = 2^-24 the partial of d is within ((h - 1) + 1) * u * sum |o - pilot| of the exact sum (the +1: the rounding of d itself) and the partial of d * d
    within ((h - 1) + 3) * u * sum (o - pilot)^2 (d * d carries the rounding of d twice and its own); held per tile against float64 sums of the kernel's own
    output.  The totals add the nparts partials in a fixed order: nparts - 1 more additions on each term;
  - weight gradients, one-call and deferred (a WgradBatch with one job), with a FrozenBN scale and dw pre-filled with NaN: fp32 within 2e-5 of the max, the
    same bits on a second run, and accumulate exactly old + gradient (the reducers add the finished sum to the old value in fp32);
  - every output - the statistics cases' out, sums and partial-row workspace included - is carved from a larger sentinel-filled allocation and the
    sentinel behind it must survive.
The worst error of every case is printed (pytest -s) as the ratio of the error to its bar."""
import contextlib
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_cases as cc
from _conv_cases import CASES, PRODUCTION, ConvCase, case_id, launch_geometry, out_hw, pad_of
from _parity import _close_bf16, _nhwc, _rand
from rnd_semantic_segmentation_amd import _lib

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ALPHA = float(np.float32(0.2))          # LeakyReLU slope of the discriminator (the library takes it as a float)
# With any plan switch of the family in the environment (a run of this module under an opt-in selection such as MI_IGEMM_STAGED=0 or MI_IGEMM_MT=6) the
# parity checks stay and each case prints its routes instead of asserting the names of the default plan.
SWITCHED = {k: v for k, v in os.environ.items() if k.startswith(("MI_IGEMM_", "MI_WGRAD_"))}


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import kernels
    return kernels


@contextlib.contextmanager
def _recording(K):
    K.ROUTES = set()
    try:
        yield K.ROUTES
    finally:
        K.ROUTES = None


def _route_is(rec, name, what):
    names = sorted(r.name for r in rec)
    if not SWITCHED:
        assert names == [name], (what, names)
    else:
        print("\n[conv route] %s took %s (plan switches %s: default-plan name not asserted)" % (what, names, SWITCHED))


def _carve(shape, dtype, sentinel, tail=4096):
    """A tensor of `shape` at the front of a larger allocation filled with `sentinel`, and the allocation"""
    n = int(np.prod(shape))
    big = torch.full((n + tail,), sentinel, dtype=dtype, device="cuda")
    return big[:n].view(shape), big


def _untouched(big, n, sentinel, what):
    assert bool((big[n:] == sentinel).all()), "%s: the launch wrote behind its output" % what


def _pack_bits(keep):
    """bool [..., N] -> int16 [..., N/16], bit n % 16 of word n / 16 (MI_EPI_WRITE_MASK's layout)"""
    w = (keep.view(*keep.shape[:-1], -1, 16).to(torch.int32) << torch.arange(16, device=keep.device, dtype=torch.int32)).sum(-1)
    return torch.where(w >= 32768, w - 65536, w).to(torch.int16).contiguous()


def _unpack_bits(words, N):
    w = words.to(torch.int32) & 0xFFFF
    return ((w.unsqueeze(-1) >> torch.arange(16, device=words.device, dtype=torch.int32)) & 1).bool().view(*words.shape[:-1], N)


def _bf16_ratio(got, ref):
    """worst |got - ref| over _close_bf16's bar (<= 1 passes)"""
    got, ref = got.double(), ref.double()
    tol = 2.0 ** -8 * ref.abs() + 2e-5 * float(ref.abs().max())
    return float(((got - ref).abs() / tol).max())


def _operands(c, seed):
    """x, w (fp32 master), dy of the case's conv on the CPU, NCHW / OIHW; x and dy are bf16"""
    k = c.ksize
    Ho, Wo = out_hw(c)
    x = _rand((c.B, c.Cin, c.H, c.W), seed)
    w = _rand((c.Cout, c.Cin, k, k), seed + 1, 1.0 / math.sqrt(c.Cin * k * k)).float()
    dy = _rand((c.B, c.Cout, Ho, Wo), seed + 2)
    return x, w, dy


def _conv_case(K, c):
    seed = 3000 + 11 * CASES.index(c)
    what = case_id(c)
    k, s, p, d, fl = c.ksize, c.stride, pad_of(c), c.dil, c.flags
    x, w, dy = _operands(c, seed)
    a_shape, N, (Ho, Wo) = launch_geometry(c)
    B = c.B
    M = B * Ho * Wo
    # float64 reference of the bare conv on the bf16-rounded operands, NHWC [B, Ho, Wo, N]
    wd = w.to(torch.bfloat16).cuda().double()
    if c.mode == "fwd":
        v = F.conv2d(x.cuda().double(), wd, None, s, p, d)
        a, wp = _nhwc(x).cuda(), K.pack_weight_fwd(w.cuda())
    else:
        xd = torch.zeros((B, c.Cin, c.H, c.W), dtype=torch.float64, device="cuda", requires_grad=True)
        F.conv2d(xd, wd, None, s, p, d).backward(dy.cuda().double())
        v = xd.grad
        a, wp = _nhwc(dy).cuda(), K.pack_weight_dgrad(w.cuda())
        del xd
    v = v.permute(0, 2, 3, 1).contiguous()
    assert tuple(v.shape) == (B, Ho, Wo, N)
    g = torch.Generator().manual_seed(seed + 5)
    worst = {}

    if fl == cc.STATS:
        pilot = (torch.randn(N, generator=g) * 0.1).cuda()
        out, obig = _carve((B, Ho, Wo, N), torch.bfloat16, 3.0)
        sums, sbig = _carve((2, N), torch.float32, 3.0)
        # the partial-row workspace (rows of [2][N] fp32, then the reducer's scratch): grown by a sentinel tail behind the size mi_conv_gemm_stats_workspace asks for
        need = int(_lib.lib().mi_conv_gemm_stats_workspace(M, N))
        ws = K._workspace(need + 4096, a.device, "conv_stats")
        ws[need:] = 0x5A
        with _recording(K) as rec:
            got, got_sums, fin = K.conv_gemm_stats(a, wp, (Ho, Wo), k, s, p, d, pilot, out=out, sums=sums)
        torch.cuda.synchronize()
        _route_is(rec, c.plan, what)
        assert got.data_ptr() == out.data_ptr() and got_sums.data_ptr() == sums.data_ptr()
        assert K._workspace(0, a.device, "conv_stats").data_ptr() == ws.data_ptr()
        _untouched(obig, out.numel(), 3.0, what)
        _untouched(sbig, sums.numel(), 3.0, what + " sums")
        _untouched(ws, need, 0x5A, what + " workspace")
        plan = next(iter(rec))
        worst["out"] = _bf16_ratio(out, v)
        _close_bf16(out, v.cpu(), what)
        h, nparts = 16 * plan.mt, 2 * plan.m_tiles
        assert nparts * h >= M > (nparts - 2) * h
        part = ws[:need].view(torch.float32)[:nparts * 2 * N].view(nparts, 2, N).double()
        assert nparts * 2 * N * 4 <= need
        dv = torch.zeros((nparts * h, N), dtype=torch.float64, device="cuda")
        dv[:M] = out.reshape(M, N).double() - pilot.double()
        dv = dv.view(nparts, h, N)
        s1, s2, sa = dv.sum(1), (dv * dv).sum(1), dv.abs().sum(1)
        r1 = (part[:, 0] - s1).abs() / (h * U * sa).clamp_min(1e-300)
        r2 = (part[:, 1] - s2).abs() / ((h + 2) * U * s2).clamp_min(1e-300)
        worst["tile stats"] = max(float(r1.max()), float(r2.max()))
        assert worst["tile stats"] <= 1.0, (what, float(r1.max()), float(r2.max()))
        t1 = (sums[0].double() - s1.sum(0)).abs() / ((h + nparts - 1) * U * sa.sum(0))
        t2 = (sums[1].double() - s2.sum(0)).abs() / ((h + nparts + 1) * U * s2.sum(0))
        worst["total stats"] = max(float(t1.max()), float(t2.max()))
        assert worst["total stats"] <= 1.0, (what, float(t1.max()), float(t2.max()))
        assert fin is None
        return worst

    kw = {}
    if fl & cc.SCALE_BIAS:
        scale, bias = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.5
        kw.update(scale=scale.cuda(), bias=bias.cuda())
        v = v * scale.cuda().double() + bias.cuda().double()
    if fl & cc.RESIDUAL:
        res = _nhwc(_rand((B, N, Ho, Wo), seed + 6)).cuda()
        kw.update(res=res)
        v = v + res.double()
    if fl & cc.RELU:
        kw.update(relu=True)
        v = torch.where(v > 0, v, ALPHA * v) if fl & cc.LEAKY else v.clamp_min(0)
    if fl & cc.LEAKY:
        kw.update(leaky=ALPHA)
    keep = None
    if fl & (cc.MASK | cc.BITMASK):
        keep = (torch.rand((B, Ho, Wo, N), generator=g) < 0.6).cuda()
        if fl & cc.MASK:
            src = _nhwc(_rand((B, N, Ho, Wo), seed + 7)).cuda().abs() + 0.25         # > 0 where kept; 0 and negative values where not
            kw.update(msk=torch.where(keep, src, torch.where(src > 1.0, -src, torch.zeros_like(src))).contiguous())
        else:
            kw.update(bits=_pack_bits(keep))
        v = torch.where(keep, v, ALPHA * v if fl & cc.LEAKY else torch.zeros_like(v))
    mbig = None
    if fl & cc.WRITE_MASK:
        mask_out, mbig = _carve((B, Ho, Wo, N // 16), torch.int16, 0x5A5A)
        kw.update(mask_out=mask_out)
    f32 = bool(fl & (cc.OUT_F32 | cc.ZSPLIT))
    oshape = (N // cc.ZGW, M, cc.ZGW) if fl & cc.ZSPLIT else (B, Ho, Wo, N)
    out, obig = _carve(oshape, torch.float32 if f32 else torch.bfloat16, 3.0)
    if fl & cc.ZSPLIT:
        kw.update(zsplit=cc.ZGW)
        v = v.reshape(M, N // cc.ZGW, cc.ZGW).permute(1, 0, 2).contiguous()
    elif fl & cc.OUT_F32:
        kw.update(out_f32=True)
    with _recording(K) as rec:
        got = K.conv_gemm(a, wp, (Ho, Wo), k, s, p, d, K.GATHER_FWD if c.mode == "fwd" else K.GATHER_DGRAD, out=out, **kw)
    torch.cuda.synchronize()
    _route_is(rec, c.plan, what)
    assert got.data_ptr() == out.data_ptr()
    _untouched(obig, out.numel(), 3.0, what)
    if f32:
        worst["out"] = float((out.double() - v).abs().max()) / (2e-5 * float(v.abs().max()))           # fp32 store: 2e-5 of the max
        assert worst["out"] <= 1.0, (what, worst["out"])
    else:
        worst["out"] = _bf16_ratio(out, v)
        _close_bf16(out, v.cpu(), what)                                                                # 1 ulp + 2e-5 of the max
    if fl & cc.WRITE_MASK:
        _untouched(mbig, mask_out.numel(), 0x5A5A, what + " mask_out")
        wrong = int((_unpack_bits(mask_out, N) != (out > 0)).sum())
        assert wrong == 0, "%s: %d sign bits differ from (stored output > 0)" % (what, wrong)
    if keep is not None and not fl & cc.LEAKY:
        assert bool((out[~keep] == 0).all()), "%s: outputs under a cleared mask bit are not exactly zero" % what
    return worst


def _wgrad_case(K, c):
    seed = 3000 + 11 * CASES.index(c)
    what = case_id(c)
    k, s, p, d = c.ksize, c.stride, pad_of(c), c.dil
    Ho, Wo = out_hw(c)
    x, w, dy = _operands(c, seed)
    xg, dyg = _nhwc(x).cuda(), _nhwc(dy).cuda()
    if c.out_map == 1:           # ASPP: row o = (branch * 9 + tap) * ncls + cls of the [O][I] product goes to dw[branch][cls][i][tap]; no FrozenBN scale
        ncls = cc.ASPP_NCLS
        G = dyg.reshape(-1, c.Cout).double().t() @ xg.reshape(-1, c.Cin).double()
        ref = G[:36 * ncls].view(4, 9, ncls, c.Cin).permute(0, 2, 3, 1).contiguous()
        shape, scale = (4, ncls, c.Cin, 3, 3), None
        ref = ref.view(shape)
    else:
        ncls = 0
        scale = torch.rand(c.Cout, generator=torch.Generator().manual_seed(seed + 4)) + 0.5
        wd = w.to(torch.bfloat16).cuda().double().requires_grad_(True)
        F.conv2d(x.cuda().double(), wd, None, s, p, d).backward(dy.cuda().double())
        ref = wd.grad * scale.cuda().double().view(-1, 1, 1, 1)
        shape, scale = tuple(w.shape), scale.cuda()
        del wd
    gmax = float(ref.abs().max())
    n = int(np.prod(shape))
    worst = {}

    def run(dw, acc, deferred):
        batch = K.WgradBatch() if deferred else None
        K.conv_wgrad(dyg, xg, dw, k, s, p, d, scale=scale, accumulate=acc, out_map=c.out_map, ncls=ncls, batch=batch)
        if batch is not None:
            batch.flush()

    for deferred, name in ((False, c.plan), (True, c.plan_deferred)):
        kind = "deferred" if deferred else "one-call"
        dw, big = _carve(shape, torch.float32, float("nan"))
        big[n:] = 9.0
        with _recording(K) as rec:
            run(dw, False, deferred)
        torch.cuda.synchronize()
        _route_is(rec, name, what + " " + kind)
        assert bool((big[n:] == 9.0).all()), "%s %s: the launch wrote behind dw" % (what, kind)
        worst[kind] = float((dw.double() - ref).abs().max()) / (2e-5 * gmax)              # fp32: 2e-5 of the max (a NaN left behind fails here)
        assert worst[kind] <= 1.0, (what, kind, worst[kind])
        dw2 = torch.full(shape, float("nan"), device="cuda")
        run(dw2, False, deferred)
        old = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda() * gmax
        acc = old.clone()
        run(acc, True, deferred)
        torch.cuda.synchronize()
        assert torch.equal(dw, dw2), "%s %s: not bit-reproducible" % (what, kind)
        assert torch.equal(acc, old + dw), "%s %s: accumulate is not old + gradient" % (what, kind)
    return worst


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_route_against_float64(K, case):
    worst = _conv_case(K, case) if isinstance(case, ConvCase) else _wgrad_case(K, case)
    print("\n[conv route] %-58s %s" % (case_id(case), "  ".join("%s %.3f" % kv for kv in worst.items())))


def test_production_routes_have_parity_cases(K, tmp_path):
    """Repeat the recording behind PRODUCTION - one eager training step of bench.py's default, deeplab_bn and fada workloads (tests/_conv_record.py) - and
    require every route it launches to be in PRODUCTION: a route production starts launching needs a case in CASES."""
    import _conv_record
    seen = _conv_record.record_production(K, str(tmp_path))
    for wl, names in seen.items():
        assert names, wl
        if not SWITCHED:
            assert names <= PRODUCTION, "%s launches routes without a parity case in tests/_conv_cases.py: %s" % (wl, sorted(names - PRODUCTION))
        else:
            print("\n[conv route] %s launches %s (plan switches %s: not compared with PRODUCTION)" % (wl, sorted(names), SWITCHED))
