"""GPU parity of the view-based kernels of the PraNet path (csrc/gconv.hip, csrc/gnet.hip) through the C-ABI, each against the torch
op the reference calls (core/models/classifiers/pranet/PraNet_Res2Net.py, Res2Net_v1b.py) evaluated in float64 on the SAME bf16-rounded
operands.  bf16 outputs: within one bf16 ulp of the exact value (2^-8 relative) plus the fp32-accumulation noise; fp32 outputs: 2e-5 of
the tensor's range.  Every case runs on channel-slice views of wider tensors where the network does."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _parity import _close_bf16, _embed, _nhwc, _rand

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gk():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import gk as g
    return g


CONV_CASES = [
    # Cin, Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), B, H, W, (ld_in, off_in), (ld_out, off_out)
    (26, 26, (3, 3), (1, 1), (1, 1), (1, 1), 2, 13, 11, (104, 26), (104, 52)),       # Res2Net group conv on a split / into a cat
    (52, 52, (3, 3), (2, 2), (1, 1), (1, 1), 2, 14, 10, (208, 52), (208, 0)),        # 'stage' block: stride 2
    (3, 32, (3, 3), (2, 2), (1, 1), (1, 1), 2, 18, 22, (3, 0), (32, 0)),             # stem conv on the image (odd alignment)
    (32, 32, (1, 7), (1, 1), (0, 3), (1, 1), 2, 9, 12, (32, 0), (32, 0)),            # RFB 1x7
    (32, 32, (7, 1), (1, 1), (3, 0), (1, 1), 2, 9, 12, (32, 0), (128, 96)),          # RFB 7x1
    (32, 32, (3, 3), (1, 1), (7, 7), (7, 7), 2, 11, 11, (32, 0), (128, 32)),         # RFB dilation 7 into the cat
    (256, 256, (5, 5), (1, 1), (2, 2), (1, 1), 1, 11, 11, (256, 0), (256, 0)),       # reverse-attention 5x5
    (128, 208, (1, 1), (1, 1), (0, 0), (1, 1), 2, 12, 12, (128, 0), (208, 0)),       # conv1 of a bottleneck: N = 208
    (104, 256, (1, 1), (1, 1), (0, 0), (1, 1), 3, 17, 9, (104, 0), (256, 0)),        # conv3
    (96, 96, (3, 3), (1, 1), (1, 1), (1, 1), 2, 12, 12, (96, 0), (96, 0)),           # partial decoder
    (64, 1, (3, 3), (1, 1), (1, 1), (1, 1), 2, 12, 12, (64, 0), (1, 0)),             # one-channel side output
    (142, 68, (3, 3), (1, 1), (1, 1), (1, 1), 2, 12, 14, (142, 0), (262, 64)),       # HarDNet, 4-byte aligned views: 32-wide tiles, two wave groups, both ways
    (40, 14, (3, 3), (1, 1), (1, 1), (1, 1), 2, 12, 14, (64, 24), (78, 64)),         # HarDNet: 16-wide tile forward, 32-wide data gradient
]
# The routes the commented rows claim (forward, data gradient).  These small maps stay below MI_GCONV_BN32_WGS / the 384-workgroup demotion, so the
# 80 / 112 / 64-wide tiles are not theirs: tests/_gconv_cases.py holds a case for every route the bench workloads launch.  Checked on the host
# by tests/test_host_gconv_routes.py.
CONV_CASE_ROUTES = {
    11: ("gconv_kernel<32, 64, 4, 4, false, false, 2>", "gconv_kernel<32, 64, 4, 4, false, false, 2>"),
    12: ("gconv_kernel<16, 64, 8, 4, false, false, 1>", "gconv_kernel<32, 32, 4, 8, false, false, 1>"),
}


def _conv_setup(case, seed):
    Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = case
    x = _rand((B, Cin, H, W), seed)
    w = _rand((Cout, Cin) + k, seed + 1, 1.0 / np.sqrt(Cin * k[0] * k[1])).float()
    geom = k + s + p + d
    return x, w, geom


@pytest.mark.parametrize("case", CONV_CASES)
def test_gconv_forward_and_batch_statistics(gk, case):
    Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = case
    x, w, geom = _conv_setup(case, 100 + Cin)
    wq = w.to(torch.bfloat16)
    ref = F.conv2d(x.double(), wq.double(), None, s, p, d)
    xv_big, xv = _embed(_nhwc(x).cuda(), ldi, offi)
    wp, _ = gk.gconv_pack(w.cuda())
    Ho, Wo = ref.shape[2], ref.shape[3]
    obig = torch.full((B, Ho, Wo, ldo), 3.0, dtype=torch.bfloat16, device="cuda")
    out, st = gk.gconv(xv, wp, Cout, geom, out=obig[..., offo:offo + Cout], stats=True)
    torch.cuda.synchronize()
    _close_bf16(out.permute(0, 3, 1, 2), ref, "conv %s" % (case,))
    rest = torch.cat([obig[..., :offo], obig[..., offo + Cout:]], -1)
    assert bool((rest == 3.0).all()), "the conv wrote outside its channel slice"
    # statistics of the ROUNDED outputs, tile partials summed here
    tiles = st.numel() // (2 * Cout)
    st = st.view(tiles, 2, Cout).double().sum(0).cpu()
    o64 = out.double().cpu().reshape(-1, Cout)
    assert torch.allclose(st[0], o64.sum(0), rtol=1e-5, atol=1e-4 * float(o64.abs().max()))
    assert torch.allclose(st[1], (o64 * o64).sum(0), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", [CONV_CASES[0], CONV_CASES[4], CONV_CASES[6], CONV_CASES[7], (104, 104, (3, 3), (1, 1), (1, 1), (1, 1), 16, 22, 22, (416, 104), (416, 208)),
                                  (64, 256, (3, 3), (1, 1), (1, 1), (1, 1), 4, 45, 45, (64, 0), (256, 0))])         # (64-wide tiles, two wave groups: 64 x 4 workgroups)
def test_conv_with_in_launch_batchnorm_finalize_equals_the_two_launch_path(gk, case):
    """mi_gconv_bn (the launch's last workgroup per column tile finalizes the BatchNorm statistics: sc1 hand-off + ticket, mi_common.h) against
    mi_gconv + mi_gbn_finalize on the same operands: the conv output, mean / invstd / scale / shift and the updated running statistics must be the
    SAME BITS (same sums in the same order), three times in a row on the same ticket words (they are left zero), incl. a 61-row-tile launch."""
    Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = case
    x, w, geom = _conv_setup(case, 300 + Cin)
    _, xv = _embed(_nhwc(x).cuda(), ldi, offi)
    wp, _ = gk.gconv_pack(w.cuda())
    g = torch.Generator().manual_seed(Cout)
    gamma, beta = (torch.rand(Cout, generator=g) + 0.5).cuda(), (torch.randn(Cout, generator=g) * 0.1).cuda()
    bias = (torch.randn(Cout, generator=g) * 0.1).cuda() if Cout % 2 else None
    Ho, Wo = gk.conv_out_hw(H, W, *geom)
    assert gk.gconv_bn_fits(B, Ho, Wo)
    rm0, rv0 = torch.randn(Cout, generator=g).cuda(), (torch.rand(Cout, generator=g) + 0.5).cuda()
    rm_a, rv_a = rm0.clone(), rv0.clone()
    y_a, st = gk.gconv(xv, wp, Cout, geom, bias=bias, stats=True)
    fin_a = gk.gbn_finalize(st, Cout, B * Ho * Wo, gamma, beta, rm_a, rv_a, 0.1, 1e-5)
    for rep in range(3):
        rm_b, rv_b = rm0.clone(), rv0.clone()
        y_b, fin_b = gk.gconv_bn(xv, wp, Cout, geom, gamma, beta, rm_b, rv_b, 0.1, 1e-5, bias=bias)
        torch.cuda.synchronize()
        assert torch.equal(y_a, y_b) and torch.equal(fin_a, fin_b), (rep, float((fin_a - fin_b).abs().max()))
        assert torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b)
        assert int(gk.tickets(xv.device).abs().sum()) == 0


def test_gconv_fp32_output_with_bias(gk):
    """agg.conv5 = nn.Conv2d(96, 1, 1) with bias (PraNet_Res2Net.py:77) and the one-channel side maps: fp32 store, no rounding."""
    x = _rand((2, 96, 12, 12), 5)
    w = _rand((1, 96, 1, 1), 6, 0.1).float()
    b = torch.tensor([0.37])
    ref = F.conv2d(x.double(), w.to(torch.bfloat16).double(), b.double())
    wp, _ = gk.gconv_pack(w.cuda())
    out, _ = gk.gconv(_nhwc(x).cuda(), wp, 1, (1, 1, 1, 1, 0, 0, 1, 1), bias=b.cuda(), out_f32=True)
    assert out.dtype == torch.float32
    assert float((out.permute(0, 3, 1, 2).double().cpu() - ref).abs().max()) < 2e-5 * float(ref.abs().max())


@pytest.mark.parametrize("case", CONV_CASES)
def test_gconv_data_and_weight_gradient(gk, case):
    Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = case
    x, w, geom = _conv_setup(case, 300 + Cin)
    xd = x.double().requires_grad_(True)
    wd = w.to(torch.bfloat16).double().requires_grad_(True)
    y = F.conv2d(xd, wd, None, s, p, d)
    dy = _rand(tuple(y.shape), 17)
    y.backward(dy.double())
    _, wpt = gk.gconv_pack(w.cuda())
    dbig, dyv = _embed(_nhwc(dy).cuda(), ldo, offo)
    xbig, xv = _embed(_nhwc(x).cuda(), ldi, offi)
    if Cin != 3:                         # the image needs no gradient
        gbig = torch.full((B, H, W, ldi), 5.0, dtype=torch.bfloat16, device="cuda")
        dx, _ = gk.gconv(dyv, wpt, Cin, geom, out=gbig[..., offi:offi + Cin], mode=gk.GATHER_DGRAD, out_hw=(H, W))
        torch.cuda.synchronize()
        _close_bf16(dx.permute(0, 3, 1, 2), xd.grad, "dgrad %s" % (case,))
    dw = torch.empty_like(w, device="cuda")
    gk.gconv_wgrad(dyv, xv, dw, geom)
    got = dw.double().cpu()
    err = float((got - wd.grad).abs().max()) / float(wd.grad.abs().max())
    assert err < 2e-5, "wgrad %s: %.3e" % (case, err)
    gk.gconv_wgrad(dyv, xv, dw, geom, accumulate=True)
    assert float((dw.double().cpu() - 2 * wd.grad).abs().max()) / float(wd.grad.abs().max()) < 4e-5


def test_fused_row_weight_gradient_on_a_large_map(gk):
    """From 65 536 output pixels up a three-column kernel at stride 1 takes gwgrad3_kernel (one staged x window for the three taps of a kernel row,
    row-wrap handled by validity bits on the dy side): 2 x 26 x 192 x 200 on channel-slice views, dilation 1 and 3, against torch in float64;
    bit-reproducible; the per-tap kernel (small maps, MI_GWGRAD3=0) is covered by the cases above and by tests/test_gpu_scripts.py."""
    for dil in (1, 3):
        case = (26, 20, (3, 3), (1, 1), (dil, dil), (dil, dil), 2, 192, 200, (104, 26), (52, 12))
        Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = case
        x, w, geom = _conv_setup(case, 700 + dil)
        xd, wd = x.double(), w.to(torch.bfloat16).double().requires_grad_(True)
        y = F.conv2d(xd, wd, None, s, p, d)
        dy = _rand(tuple(y.shape), 19)
        y.backward(dy.double())
        _, dyv = _embed(_nhwc(dy).cuda(), ldo, offo)
        _, xv = _embed(_nhwc(x).cuda(), ldi, offi)
        dw, dw2 = torch.empty_like(w, device="cuda"), torch.empty_like(w, device="cuda")
        gk.gconv_wgrad(dyv, xv, dw, geom)
        gk.gconv_wgrad(dyv, xv, dw2, geom)
        torch.cuda.synchronize()
        err = float((dw.double().cpu() - wd.grad).abs().max()) / float(wd.grad.abs().max())
        assert err < 2e-5, (dil, err)
        assert torch.equal(dw, dw2)


def test_kernel_row_window_conv_on_a_large_map(gk):
    """From 512 64-wide workgroups up a stride-1 conv with three kernel columns, pad = dilation and >= 4 chunks per kernel row takes gconv3_kernel (one staged
    window of 128 + 2 d pixels per kernel row and 32-channel chunk, the three taps' MFMAs from it; row wrap by validity bits, image borders by zero window rows):
    2 x 136 x 200 x 168 -> 136 on channel-slice views (both directions five chunks per kernel row, 80-wide tiles), dilation 1 and 3, forward (+ the column
    statistics) and data gradient against torch in float64.  The
    tiny shapes run through it in tests/test_gpu_scripts.py (MI_GCONV3_WGS=1)."""
    for dil in (1, 3):
        case = (136, 136, (3, 3), (1, 1), (dil, dil), (dil, dil), 2, 200, 168, (272, 136), (144, 8))
        Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = case
        x, w, geom = _conv_setup(case, 800 + dil)
        xd = x.double().requires_grad_(True)
        wd = w.to(torch.bfloat16).double()
        y = F.conv2d(xd, wd, None, s, p, d)
        dy = _rand(tuple(y.shape), 23)
        y.backward(dy.double())
        wp, wpt = gk.gconv_pack(w.cuda())
        _, xv = _embed(_nhwc(x).cuda(), ldi, offi)
        obig = torch.zeros((B, H, W, ldo), dtype=torch.bfloat16, device="cuda")
        out, st = gk.gconv(xv, wp, Cout, geom, out=obig[..., offo:offo + Cout], stats=True)
        torch.cuda.synchronize()
        _close_bf16(out.permute(0, 3, 1, 2), y.detach(), "window conv forward d=%d" % dil)
        assert float(obig[..., :offo].abs().max()) == 0.0                      # nothing outside the slice is written
        tiles = (B * H * W + 127) // 128
        sums = st.view(tiles, 2, Cout).double().sum(0).cpu()
        yb = out.permute(0, 3, 1, 2).double().cpu()
        assert float((sums[0] - yb.sum((0, 2, 3))).abs().max()) < 1e-3 * float(yb.abs().sum((0, 2, 3)).max())
        assert float((sums[1] - (yb * yb).sum((0, 2, 3))).abs().max()) < 1e-3 * float((yb * yb).sum((0, 2, 3)).max())
        _, dyv = _embed(_nhwc(dy).cuda(), ldo, offo)
        dx, _ = gk.gconv(dyv, wpt, Cin, geom, mode=gk.GATHER_DGRAD, out_hw=(H, W))
        torch.cuda.synchronize()
        _close_bf16(dx.permute(0, 3, 1, 2), xd.grad, "window conv data gradient d=%d" % dil)


def test_weight_gradients_of_many_convs_in_one_launch(gk):
    """gk.gconv_wgrad_multi (the tape's end-of-backward flush): every conv case of this file - all operand alignment classes, strides, dilations, 1 x 7 /
    7 x 1 / 5 x 5 kernels, the fused kernel row where the geometry allows it - plus a 16 x 44 x 44 map with several K splits, queued together; each gradient
    against torch in float64, accumulate on half of them, and the whole call twice: the same bits."""
    jobs, refs, keep = [], [], []
    cases = list(CONV_CASES) + [(52, 52, (3, 3), (1, 1), (1, 1), (1, 1), 16, 44, 44, (208, 52), (52, 0)), (104, 104, (3, 3), (1, 1), (1, 1), (1, 1), 4, 22, 22, (104, 0), (104, 0))]
    for n, case in enumerate(cases):
        Cin, Cout, k, s, p, d, B, H, W, (ldi, offi), (ldo, offo) = case
        x, w, geom = _conv_setup(case, 900 + n)
        wd = w.to(torch.bfloat16).double().requires_grad_(True)
        y = F.conv2d(x.double(), wd, None, s, p, d)
        dy = _rand(tuple(y.shape), 40 + n)
        y.backward(dy.double())
        _, dyv = _embed(_nhwc(dy).cuda(), ldo, offo)
        _, xv = _embed(_nhwc(x).cuda(), ldi, offi)
        acc = n % 2 == 1
        dw = torch.full(tuple(w.shape), 0.25 if acc else float("nan"), device="cuda")
        jobs.append((dyv, xv, dw, geom, acc))
        refs.append(wd.grad + (0.25 if acc else 0.0))
        keep.append((dyv, xv))
    gk.gconv_wgrad_multi(jobs)
    torch.cuda.synchronize()
    first = [j[2].clone() for j in jobs]
    for case, j, ref in zip(cases, jobs, refs):
        err = float((j[2].double().cpu() - ref).abs().max()) / float(ref.abs().max())
        assert err < 2e-5, "multi wgrad %s: %.3e" % (case, err)
    for j in jobs:
        j[2].fill_(0.25 if j[4] else float("nan"))
    gk.gconv_wgrad_multi(jobs)
    torch.cuda.synchronize()
    assert all(torch.equal(a, j[2]) for a, j in zip(first, jobs))
    with pytest.raises(Exception, match="same gradient"):
        gk.gconv_wgrad_multi([jobs[0], jobs[0]])


def test_gconv_weight_gradient_is_bit_reproducible_and_splits_k(gk):
    """M = 16 x 44 x 44 pixels: several K splits; two runs give the same bits (fixed-order slab reduction)."""
    x = _rand((16, 52, 44, 44), 1)
    dy = _rand((16, 52, 44, 44), 2)
    dw1 = torch.empty((52, 52, 3, 3), device="cuda")
    dw2 = torch.empty_like(dw1)
    geom = (3, 3, 1, 1, 1, 1, 1, 1)
    a, b = _nhwc(dy).cuda(), _nhwc(x).cuda()
    gk.gconv_wgrad(a, b, dw1, geom)
    gk.gconv_wgrad(a, b, dw2, geom)
    assert torch.equal(dw1, dw2)
    ref = torch.nn.grad.conv2d_weight(x.float().cuda(), (52, 52, 3, 3), dy.float().cuda(), 1, 1, 1)
    assert float((dw1 - ref).abs().max()) / float(ref.abs().max()) < 1e-4


@pytest.mark.parametrize("C,relu,with_add,f32", [(26, True, False, False), (104, True, True, False), (32, False, False, False), (1, False, False, True),
                                                 (256, True, False, False), (104, 6, False, False), (26, 6, False, False), (32, 6, False, True)])
def test_batchnorm_train_forward_backward(gk, C, relu, with_add, f32):
    """conv statistics -> mi_gbn_finalize -> mi_gbn_apply, and the two backward kernels, against nn.BatchNorm2d in train() (float64).  relu: False,
    True or 6 (ReLU6 = F.hardtanh(., 0, 6), activation code 2 as conv_bn passes it; gamma / beta put over a third of the outputs above 6 and some
    within one bf16 ulp of it; bf16 g on VEC 8 / VEC 2 channel counts and an fp32 g).  The kernels mask the gradient by the STORED output; that
    mask may differ from torch's only where the float64 pre-activation lies within one bf16 ulp of 0 or 6 - asserted, and inside that band the
    reference takes the kernel's mask."""
    B, H, W = 3, 13, 9
    x = _rand((B, max(C, 8), H, W), 40 + C)
    w = _rand((C, max(C, 8), 1, 1), 41 + C, 0.3).float()
    wp, _ = gk.gconv_pack(w.cuda())
    y, st = gk.gconv(_nhwc(x).cuda(), wp, C, (1, 1, 1, 1, 0, 0, 1, 1), stats=True)          # y: bf16 conv output + tile statistics
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(2, 4, C) if relu == 6 else torch.linspace(0.5, 1.5, C))
        bn.bias.copy_(torch.linspace(4.5, 5.5, C) if relu == 6 else torch.linspace(-0.3, 0.4, C))
        bn.running_mean.copy_(torch.linspace(-1, 1, C))
        bn.running_var.copy_(torch.linspace(0.5, 2, C))
    rm, rv = bn.running_mean.float().cuda(), bn.running_var.float().cuda()
    yd = y.permute(0, 3, 1, 2).double().cpu().requires_grad_(True)
    add = _rand((B, C, H, W), 43) if with_add else None
    pre = bn(yd)
    if add is not None:
        pre = pre + add.double()
    ref = F.hardtanh(pre, 0.0, 6.0) if relu == 6 else (F.relu(pre) if relu else pre)
    g = _rand((B, C, H, W), 44)
    if f32:
        g = g.float() * 1.37
    fin = gk.gbn_finalize(st, C, B * H * W, bn.weight.float().cuda(), bn.bias.float().cuda(), rm, rv, 0.1, 1e-5)
    mean, invstd, scale, shift = fin[0], fin[1], fin[2], fin[3]
    addv = _embed(_nhwc(add).cuda(), C + 6, 4)[1] if add is not None else None
    out = gk.gbn_apply(y, scale, shift, 2 if relu == 6 else int(bool(relu)), add=addv, out_f32=f32)
    torch.cuda.synchronize()
    if f32:
        assert float((out.permute(0, 3, 1, 2).double().cpu() - ref.detach()).abs().max()) < 2e-5 * float(ref.abs().max()) + 1e-5
    else:
        _close_bf16(out.permute(0, 3, 1, 2), ref.detach(), "bn apply C=%d" % C, floor=1e-4)
    assert torch.allclose(rm.double().cpu(), bn.running_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rv.double().cpu(), bn.running_var, rtol=1e-4, atol=1e-6)
    if relu:
        # mask agreement: near 0 the band is one bf16 ulp of the magnitudes that cancel (|gamma xhat| + |beta| + |add|), at 6 one ulp of 6 (2^-5)
        o, p = out.permute(0, 3, 1, 2).double().cpu(), pre.detach()
        hi = 6.0 if relu == 6 else float("inf")
        beta = bn.bias.detach().view(1, C, 1, 1)
        a64 = add.double() if add is not None else torch.zeros_like(p)
        mag = (p - beta - a64).abs() + beta.abs() + a64.abs()
        band = (p.abs() <= 2.0 ** -8 * mag) | ((p - 6.0).abs() <= 2.0 ** -5 if relu == 6 else torch.zeros_like(p, dtype=torch.bool))
        mk, mt = (o > 0) & (o < hi), (p > 0) & (p < hi)
        flip = mk != mt
        print("bn C=%d relu=%s: %d of %d above the clamp, %d in the one-ulp band, %d masks differ (bar: none outside the band)"
              % (C, relu, int((p >= 6).sum()) if relu == 6 else 0, p.numel(), int(band.sum()), int(flip.sum())))
        assert not bool((flip & ~band).any()), "the kernels' gradient mask differs from torch's outside the one-ulp band"
        pre.backward(g.double() * torch.where(band, mk, mt))
    else:
        pre.backward(g.double())
    # backward: the ReLU / ReLU6 mask comes from the stored output
    gv = _nhwc(g).cuda()
    dbeta, dgamma = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    mask = out if relu else None
    gk.gbn_bwd_sums(gv, y, mask, mean, invstd, dbeta, dgamma, relu6=relu == 6)
    dy = gk.gbn_bwd_apply(gv, y, mask, mean, invstd, bn.weight.float().cuda(), dbeta, dgamma, B * H * W, relu6=relu == 6)
    torch.cuda.synchronize()
    assert torch.allclose(dbeta.double().cpu(), bn.bias.grad, rtol=2e-3, atol=2e-3 * float(bn.bias.grad.abs().max()))
    assert torch.allclose(dgamma.double().cpu(), bn.weight.grad, rtol=2e-3, atol=2e-3 * float(bn.weight.grad.abs().max()))
    e = float((dy.permute(0, 3, 1, 2).double().cpu() - yd.grad).abs().max()) / float(yd.grad.abs().max())
    assert e < 1.5e-2, e                # bf16 dy (2^-8) on top of the mask agreement


def test_batchnorm_apply_refuses_unknown_activation_codes(gk):
    """The applies take an activation CODE (0 none, 1 ReLU, 2 ReLU6); 6 - what gconv_f32's relu=6 means - or any other value is refused instead of
    running as a plain ReLU."""
    from rnd_semantic_segmentation_amd._lib import MiError
    y = _nhwc(_rand((1, 16, 3, 3), 7)).cuda()
    sc, sh = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
    for code in (6, 3, -1):
        with pytest.raises(MiError, match="activation code"):
            gk.gbn_apply(y, sc, sh, code)
        with pytest.raises(MiError, match="activation code"):
            gk.gbn_apply_multi(y, sc, sh, code, [])
    assert torch.equal(gk.gbn_apply(y, sc, sh, 2), y.clamp(0, 6))


def test_bias_gradient_is_a_column_sum(gk):
    g = torch.randn(2, 12, 12, 1, device="cuda")
    db = torch.zeros(1, device="cuda")
    gk.gbn_bwd_sums(g, None, None, None, None, db, None)
    assert abs(float(db) - float(g.double().sum())) < 1e-4


@pytest.mark.parametrize("k,s,p,inc,H,W", [(3, 1, 1, True, 9, 11), (3, 2, 1, True, 12, 10), (2, 2, 0, False, 12, 10), (2, 2, 0, False, 13, 9)])
def test_average_pools(gk, k, s, p, inc, H, W):
    """AvgPool2d(3, stride, 1) of the 'stage' blocks and AvgPool2d(s, s, ceil_mode=True, count_include_pad=False) of the downsample path."""
    C = 26
    x = _rand((2, C, H, W), 60)
    xd = x.double().requires_grad_(True)
    ref = F.avg_pool2d(xd, k, s, p, ceil_mode=not inc, count_include_pad=inc)
    g = _rand(tuple(ref.shape), 61)
    ref.backward(g.double())
    xbig, xv = _embed(_nhwc(x).cuda(), 104, 78)
    out = gk.gavgpool(xv, k, s, p, inc, (ref.shape[2], ref.shape[3]))
    _close_bf16(out.permute(0, 3, 1, 2), ref.detach(), "avgpool")
    dx = gk.gavgpool_bwd(_nhwc(g).cuda(), (H, W), k, s, p, inc)
    _close_bf16(dx.permute(0, 3, 1, 2), xd.grad, "avgpool bwd")


@pytest.mark.parametrize("H,W,sf,align,f32", [(11, 11, 32, False, True), (44, 44, 0.25, False, True), (11, 11, 2, False, True), (12, 9, 8, False, True),
                                               (6, 5, 2, True, False), (3, 3, 2, True, False), (9, 7, 2, False, False), (16, 12, 0.5, False, False),
                                               (5, 6, 4, False, False)])
def test_bilinear_resize_both_conventions(gk, H, W, sf, align, f32):
    """F.interpolate(scale_factor=..., mode='bilinear') with align_corners False (PraNet_Res2Net.py:127-177) on fp32 one-channel maps and
    nn.Upsample(scale_factor=2, align_corners=True) (:67) on bf16 feature maps; forward and backward."""
    C = 1 if f32 else 32
    x = _rand((2, C, H, W), 70)
    x = x.float() if f32 else x
    xd = x.double().requires_grad_(True)
    ref = F.interpolate(xd, scale_factor=sf, mode="bilinear", align_corners=align)
    g = _rand(tuple(ref.shape), 71)
    g = g.float() if f32 else g
    ref.backward(g.double())
    out = gk.gresize(_nhwc(x).cuda(), (ref.shape[2], ref.shape[3]), align, sf)
    dx = gk.gresize_bwd(_nhwc(g).cuda(), (H, W), align, sf)
    torch.cuda.synchronize()
    if f32:
        assert float((out.permute(0, 3, 1, 2).double().cpu() - ref.detach()).abs().max()) < 1e-5
        assert float((dx.permute(0, 3, 1, 2).double().cpu() - xd.grad).abs().max()) < 1e-5 * max(1.0, float(xd.grad.abs().max()))
    else:
        _close_bf16(out.permute(0, 3, 1, 2), ref.detach(), "resize")
        _close_bf16(dx.permute(0, 3, 1, 2), xd.grad, "resize bwd")


def test_resize_to_a_given_size(gk):
    """pranet_tester.py:39: F.upsample(output, size=(h, w), mode='bilinear', align_corners=False) - scale = in / out."""
    x = torch.randn(1, 1, 88, 88)
    ref = F.interpolate(x, size=(300, 211), mode="bilinear", align_corners=False)
    out = gk.gresize(_nhwc(x).cuda(), (300, 211), False, None)
    assert float((out.permute(0, 3, 1, 2).cpu() - ref).abs().max()) < 1e-5


def test_elementwise_and_reverse_attention(gk):
    a, b = _rand((2, 26, 7, 9), 80), _rand((2, 26, 7, 9), 81)
    abig, av = _embed(_nhwc(a).cuda(), 104, 26)
    bv = _nhwc(b).cuda()
    _close_bf16(gk.gbinary(gk.OP_ADD, av, bv).permute(0, 3, 1, 2), a.double() + b.double(), "add")
    _close_bf16(gk.gbinary(gk.OP_MUL, av, bv).permute(0, 3, 1, 2), a.double() * b.double(), "mul")
    _close_bf16(gk.gbinary(gk.OP_RELU_MASK, av, bv).permute(0, 3, 1, 2), torch.where(b > 0, a, torch.zeros_like(a)).double(), "mask")
    assert torch.equal(gk.gbinary(gk.OP_COPY, av).cpu(), _nhwc(a))
    # OP_MULRELU (FAM's relu(a * b)): on the 2-byte-offset view above (VEC 2), a 64-channel pair (VEC 8) and an odd channel offset (VEC 1)
    _close_bf16(gk.gbinary(gk.OP_MULRELU, av, bv).permute(0, 3, 1, 2), F.relu(a.double() * b.double()), "mulrelu VEC 2")
    a8, b8 = _rand((2, 64, 7, 9), 84), _rand((2, 64, 7, 9), 85)
    _close_bf16(gk.gbinary(gk.OP_MULRELU, _nhwc(a8).cuda(), _nhwc(b8).cuda()).permute(0, 3, 1, 2), F.relu(a8.double() * b8.double()), "mulrelu VEC 8")
    _, a1 = _embed(_nhwc(a).cuda(), 104, 27)
    _close_bf16(gk.gbinary(gk.OP_MULRELU, a1, bv).permute(0, 3, 1, 2), F.relu(a.double() * b.double()), "mulrelu VEC 1")
    f = torch.randn(2, 7, 9, 1, device="cuda")
    assert torch.equal(gk.gbinary(gk.OP_COPY, f, out_dtype=torch.bfloat16), f.to(torch.bfloat16))
    # reverse attention
    feat = _rand((2, 64, 7, 9), 82)
    gate = torch.randn(2, 1, 7, 9)
    fd, gd = feat.double().requires_grad_(True), gate.double().requires_grad_(True)
    ref = (-1 * torch.sigmoid(gd) + 1).expand(-1, 64, -1, -1).mul(fd)
    dy = _rand((2, 64, 7, 9), 83)
    ref.backward(dy.double())
    gt = _nhwc(gate).cuda()
    out = gk.gra_fwd(gt, _nhwc(feat).cuda())
    _close_bf16(out.permute(0, 3, 1, 2), ref.detach(), "reverse attention")
    dfeat, dgate = gk.gra_bwd(gt, _nhwc(feat).cuda(), _nhwc(dy).cuda())
    _close_bf16(dfeat.permute(0, 3, 1, 2), fd.grad, "reverse attention dfeat")
    assert float((dgate.permute(0, 3, 1, 2).double().cpu() - gd.grad).abs().max()) < 1e-4 * float(gd.grad.abs().max()) + 1e-5


@pytest.mark.parametrize("C,ranges,relu", [(104, [(78, 104, False), (0, 26, True)], 1), (40, [(0, 40, False), (0, 40, False), (8, 24, True)], 2),
                                           (256, [(0, 256, True), (64, 128, False), (0, 8, False), (248, 256, True)], 0)])
def test_batchnorm_apply_with_extra_destinations_equals_the_separate_launches(gk, C, ranges, relu):
    """mi_gbn_apply_multi: channel ranges of the result, as stored, also go to other views in the same launch - optionally plus a second operand.  Against
    mi_gbn_apply followed by the copy / add launches it replaces (mi_gbinary on the stored tensor): EQUAL BIT FOR BIT, for 2-byte (26-channel Res2Net groups),
    16-byte and mixed alignments, channel-slice views on both sides, with and without the residual operand of the apply itself."""
    B, H, W = 2, 9, 7
    dev = "cuda"
    y = _nhwc(_rand((B, C, H, W), 3)).to(dev).to(torch.bfloat16)
    sc = (_rand((C,), 4).float() * 0.5 + 1.0).to(dev)
    sh = _rand((C,), 5).float().to(dev)
    res = _nhwc(_rand((B, C, H, W), 6)).to(dev).to(torch.bfloat16) if relu != 2 else None
    want_out = gk.gbn_apply(y, sc, sh, relu, add=res)
    extras, want = [], []
    for k, (c0, c1, with_add) in enumerate(ranges):
        wide = torch.full((B, H, W, (c1 - c0) + 6), 7.0, dtype=torch.bfloat16, device=dev)          # destination = a channel slice of a wider buffer
        dst = wide[..., 2:2 + (c1 - c0)] if (c1 - c0) % 8 else wide[..., :c1 - c0]
        a2 = _nhwc(_rand((B, c1 - c0, H, W), 10 + k)).to(dev).to(torch.bfloat16) if with_add else None
        extras.append((c0, c1, dst, a2))
        src = want_out[..., c0:c1]
        want.append(gk.gbinary(gk.OP_ADD, src, a2) if with_add else gk.gbinary(gk.OP_COPY, src))
    out = gk.gbn_apply_multi(y, sc, sh, relu, extras, add=res)
    torch.cuda.synchronize()
    assert torch.equal(out, want_out)
    for k, ((c0, c1, dst, a2), w) in enumerate(zip(extras, want)):
        assert torch.equal(dst, w), "extra destination %d (channels %d..%d) differs from the separate launch" % (k, c0, c1)
        full, off = dst._base, dst.storage_offset() % dst._base.shape[-1]
        assert bool((full[..., :off] == 7.0).all()) and bool((full[..., off + (c1 - c0):] == 7.0).all())        # nothing outside the view was touched
    from rnd_semantic_segmentation_amd._lib import MiError
    with pytest.raises(MiError):
        gk.gbn_apply_multi(y, sc, sh, relu, extras * 3)                                               # more than four destinations
