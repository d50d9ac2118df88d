"""Float64 parity of every general-conv route the bench workloads launch (tests/_gconv_cases.py: PRODUCTION, CASES).

Each case runs (at default switches) on channel-slice views of sentinel-filled tensors, at a shape and layout for which the dispatcher picks the route
the case names itself (asserted through gk.ROUTES), and checks against float64 torch on the same bf16-rounded operands, computed on the device:
  - the forward output (with a bias): bf16 within _parity._close_bf16 (1 ulp + 2e-5 of the max; the kernel accumulates in fp32 and rounds once),
    fp32 side maps within 2e-5 of the max; nothing outside the output slice changes;
  - the batch statistics: the epilogue sums the bf16-ROUNDED outputs of each 128-row tile in fp32 (rows of a row group in order, then the groups: 127
    additions), and v * v of a bf16 value is exact in fp32, so each tile partial is within 127 * 2^-24 * sum|y| (sum y^2) of the exact sum; held per
    tile and channel against float64 sums of the kernel's own output (the per-channel totals follow);
  - the data gradient (bf16, _close_bf16), with the same slice check;
  - the one-conv and the batched weight gradients: fp32 within 2e-5 of the max, the same bits on a second run, and the accumulate path exactly
    old + gradient (the reducers add the finished sum to the old value in fp32).
The worst error of every case is printed (pytest -s), as the ratio of the error to its bar."""
import contextlib
import math
import os

import pytest
import torch
import torch.nn.functional as F

from _gconv_cases import CASES, PRODUCTION, geom8, out_hw
from _parity import _close_bf16, _embed, _nhwc, _rand

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# The switches that change a plan (csrc/gconv.hip: gconv_plan, gwgrad_route, gwm_route).  With any of them set - tests/test_gpu_scripts.py runs cases
# under opt-in selections - the parity checks stay and each case prints its routes instead of asserting the names of the default plan.
PLAN_SWITCHES = ("MI_GCONV_BN32_WGS", "MI_GCONV_BN_ANY", "MI_GCONV_BN_C", "MI_GCONV_BN_FORCE", "MI_GCONV_BN128", "MI_GCONV_KC", "MI_GCONV_KC32_WGS",
                 "MI_GCONV_KS2_WGS", "MI_GCONV3_WGS", "MI_GWGRAD3", "MI_GWM_FUSED3", "MI_GWM_STEPS")
SWITCHED = {k: os.environ[k] for k in PLAN_SWITCHES if k in os.environ}


@pytest.fixture(scope="module")
def gk():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import gk as g
    return g


@contextlib.contextmanager
def _recording(gk):
    gk.ROUTES = set()
    try:
        yield gk.ROUTES
    finally:
        gk.ROUTES = None


def _names(routes):
    return {r.name for r in routes}


def _route_is(rec, name, *what):
    if not SWITCHED:
        assert _names(rec) == {name}, what + (sorted(_names(rec)),)
    else:
        print("\n[gconv route] %s took %s (plan switches %s: default-plan name not asserted)" % (" ".join(what), sorted(_names(rec)), SWITCHED))


def _bf16_ratio(got, ref):
    """worst |got - ref| over _close_bf16's bar (<= 1 passes)"""
    got, ref = got.double(), ref.double()
    tol = 2.0 ** -8 * ref.abs() + 2e-5 * float(ref.abs().max())
    return float(((got - ref).abs() / tol).max())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_route_against_float64(gk, case):
    Cin, Cout, B, H, W = case.Cin, case.Cout, case.B, case.H, case.W
    (ldi, offi), (ldo, offo) = case.x_view, case.y_view
    (kh, kw), s, p, d = case.geom
    geom = geom8(case)
    Ho, Wo = out_hw(case)
    seed = 1000 + 7 * CASES.index(case)
    x = _rand((B, Cin, H, W), seed)
    w = _rand((Cout, Cin, kh, kw), seed + 1, 1.0 / math.sqrt(Cin * kh * kw)).float()
    dy = _rand((B, Cout, Ho, Wo), seed + 2)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(seed + 3)) * 0.5        # (rows past M then hold the bias in the epilogue's tile)
    # float64 reference on the device, on the bf16-rounded operands
    xd = x.cuda().double().requires_grad_(True)
    wd = w.to(torch.bfloat16).cuda().double().requires_grad_(True)
    y = F.conv2d(xd, wd, None, s, p, d)
    y.backward(dy.cuda().double())
    ref_y, ref_dx, ref_dw = y.detach() + bias.cuda().double().view(1, -1, 1, 1), xd.grad, wd.grad
    del xd, wd, y
    wp, wpt = gk.gconv_pack(w.cuda())
    _, xv = _embed(_nhwc(x).cuda(), ldi, offi)
    worst = {}

    # forward (+ batch statistics)
    odt = torch.float32 if case.f32 else torch.bfloat16
    obig = torch.full((B, Ho, Wo, ldo), 3.0, dtype=odt, device="cuda")
    with _recording(gk) as rec:
        out, st = gk.gconv(xv, wp, Cout, geom, out=obig[..., offo:offo + Cout], bias=bias.cuda(), stats=not case.f32, out_f32=case.f32)
    torch.cuda.synchronize()
    _route_is(rec, case.fwd, case.name, "fwd")
    got = out.permute(0, 3, 1, 2)
    if case.f32:
        worst["fwd"] = float((got.double() - ref_y).abs().max()) / (2e-5 * float(ref_y.abs().max()))       # fp32 store: 2e-5 of the max
        assert worst["fwd"] <= 1.0, (case.name, worst["fwd"])
    else:
        worst["fwd"] = _bf16_ratio(got, ref_y)
        _close_bf16(got, ref_y.cpu(), "forward %s" % case.name)                                       # 1 ulp + 2e-5 of the max
        # per 128-row tile (the last one partial) and channel, against float64 sums of the kernel's own rounded output: 127 fp32 additions per
        # partial, so |error| <= 127 * 2^-24 * sum |y| (sum y^2: the squares are exact in fp32 and non-negative)
        tiles = (B * Ho * Wo + 127) // 128
        part = st.view(tiles, 2, Cout).double()
        yo = torch.zeros((tiles * 128, Cout), dtype=torch.float64, device="cuda")
        yo[:B * Ho * Wo] = out.reshape(-1, Cout).double()
        yo = yo.view(tiles, 128, Cout)
        sy, sy2 = yo.sum(1), (yo * yo).sum(1)
        r1 = (part[:, 0] - sy).abs() / (127 * U * yo.abs().sum(1)).clamp_min(1e-300)
        r2 = (part[:, 1] - sy2).abs() / (127 * U * sy2).clamp_min(1e-300)
        worst["stats"] = max(float(r1.max()), float(r2.max()))
        assert worst["stats"] <= 1.0, (case.name, float(r1.max()), float(r2.max()))
    rest = torch.cat([obig[..., :offo], obig[..., offo + Cout:]], -1)
    assert bool((rest == 3.0).all()), "%s: the forward wrote outside its channel slice" % case.name

    # data gradient
    _, dyv = _embed(_nhwc(dy).cuda(), ldo, offo)
    gbig = torch.full((B, H, W, ldi), 5.0, dtype=torch.bfloat16, device="cuda")
    with _recording(gk) as rec:
        dx, _ = gk.gconv(dyv, wpt, Cin, geom, out=gbig[..., offi:offi + Cin], mode=gk.GATHER_DGRAD, out_hw=(H, W))
    torch.cuda.synchronize()
    _route_is(rec, case.dgrad, case.name, "dgrad")
    worst["dgrad"] = _bf16_ratio(dx.permute(0, 3, 1, 2), ref_dx)
    _close_bf16(dx.permute(0, 3, 1, 2), ref_dx.cpu(), "data gradient %s" % case.name)                 # 1 ulp + 2e-5 of the max
    rest = torch.cat([gbig[..., :offi], gbig[..., offi + Cin:]], -1)
    assert bool((rest == 5.0).all()), "%s: the data gradient wrote outside its channel slice" % case.name

    # weight gradients: one conv, then one job of the batched launch
    gmax = float(ref_dw.abs().max())
    for kind, run in (("wgrad", lambda dw, acc: gk.gconv_wgrad(dyv, xv, dw, geom, accumulate=acc)),
                      ("wgrad_multi", lambda dw, acc: gk.gconv_wgrad_multi([(dyv, xv, dw, geom, acc)]))):
        dw = torch.full(tuple(w.shape), float("nan"), device="cuda")
        with _recording(gk) as rec:
            run(dw, False)
        torch.cuda.synchronize()
        _route_is(rec, getattr(case, kind), case.name, kind)
        worst[kind] = float((dw.double() - ref_dw).abs().max()) / (2e-5 * gmax)                         # fp32: 2e-5 of the max
        assert worst[kind] <= 1.0, (case.name, kind, worst[kind])
        dw2 = torch.full(tuple(w.shape), float("nan"), device="cuda")
        run(dw2, False)
        old = torch.randn(tuple(w.shape), generator=torch.Generator().manual_seed(seed)).cuda() * gmax
        acc = old.clone()
        run(acc, True)
        torch.cuda.synchronize()
        assert torch.equal(dw, dw2), "%s %s: not bit-reproducible" % (case.name, kind)
        assert torch.equal(acc, old + dw), "%s %s: accumulate is not old + gradient" % (case.name, kind)
    print("\n[gconv route] %-30s %s" % (case.name, "  ".join("%s %.3f" % kv for kv in worst.items())))


def test_production_routes_have_parity_cases(gk):
    """Repeat the recording behind PRODUCTION - one eager training step of PraNet (16 x 352 x 352) and of GALD (6 x 720 x 1280), built as bench.py's
    aux_workload builds them - and require every route it launches to be in PRODUCTION: a route production starts launching needs a case in CASES."""
    from rnd_semantic_segmentation_amd.host import gald, pranet, synth
    dev = torch.device("cuda")
    seen = {}
    torch.manual_seed(0)
    net = pranet.PraNet().to(dev).train()
    net.ensure_flat()
    opt = pranet.FlatAdam(net, 1e-4 / 8, grad_clamp=0.5)
    img, mask = synth.synth_polyp(16, 352, 352, seed=3)
    x, gt = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    with _recording(gk) as rec:
        opt.zero_grad()
        ls = [pranet.structure_loss(o, gt) for o in net(x)]
        (ls[3] + ls[2] + ls[1] + ls[0]).backward()
        opt.step()
        torch.cuda.synchronize()
    seen["pranet"] = _names(rec)
    del net, opt, x, gt, ls
    torch.manual_seed(0)
    enc, dec = gald.GCPAEncoder().to(dev).train(), gald.GCPADecoder().to(dev).train()
    enc.ensure_flat()
    dec.ensure_flat()
    oe, od = pranet.FlatAdam(enc, 1e-4), pranet.FlatAdam(dec, 1e-3)
    x = torch.from_numpy(synth.synth_image(6, 720, 1280, seed=9)).to(dev)
    lab = torch.from_numpy(synth.synth_label(6, 720, 1280, 19, seed=9)).to(dev).long()
    with _recording(gk) as rec:
        oe.zero_grad()
        od.zero_grad()
        l5, l4, l3, l2 = dec.losses(x, enc(x), lab)
        (l2 * 1 + l3 * 0.8 + l4 * 0.6 + l5 * 0.4).backward()
        oe.step()
        od.step()
        torch.cuda.synchronize()
    seen["gald"] = _names(rec)
    for wl, names in seen.items():
        assert names, wl
        assert names <= PRODUCTION, "%s launches routes without a parity case in tests/_gconv_cases.py: %s" % (wl, sorted(names - PRODUCTION))
