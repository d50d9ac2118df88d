"""Per-channel / per-element float64 parity of csrc/batchnorm.hip (mi_bn_colsum, mi_bn_colsum2, mi_bn_finalize, mi_bn_apply, mi_bn_bwd_colsums,
mi_bn_bwd_apply, the epilogue-partials reducer behind mi_conv_gemm_stats) and csrc/colsum.hip (mi_aspp_bias_grad, mi_bias_grad_bf16).

Unlike tests/test_gpu_bn.py (one relmax per tensor, channels of one scale) every channel here has its own scale, 2^((5c mod 13) - 6), and is compared on its
own against a bar DERIVED from the kernels' fixed summation order (tests/_bn_ref.py: depth, 2^-24, 2^-8, the operands' magnitudes; nothing measured); the
shapes are the smallest that reach each edge of bn_plan / colsum.hip's launch() (tests/_bn_ref.py bn_shapes, colsum_shapes).  tests/test_host_bn_ref.py
shows on the CPU that the kernels' order stays inside these bars and that a dropped row, a doubled row or a swapped slot does not."""
import numpy as np
import pytest
import torch

import _bn_ref as R
from rnd_semantic_segmentation_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"

BN_CASES = [(C, M, "std") for C, M in R.bn_shapes()] + [(64, 129, "pilot0"), (64, 129, "const")]
_ids = lambda v: "c%d_m%d_%s" % v


def _case(C, M, variant):
    return R.make_bn_case(C, M, variant)


def _icase(C, M):
    return R.make_int_case(C, M)


def _d(t):
    return t.to(DEV).contiguous()


def _within(name, got, ref, bar):
    """Per channel / element: |got - ref| <= bar, no exception.  Prints the worst ratio before asserting."""
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bar)                                   # a NaN is bad
    ratio = float((err / np.maximum(bar, 1e-300)).max()) if err.size else 0.0
    print("[bn parity] %-28s worst |err| / bar = %.3f" % (name, ratio))
    assert not bad.any(), "%s: %d of %d outside the bar, first at flat index %d: got %r, want %r, bar %.3e" % (
        name, int(bad.sum()), bad.size, int(np.argmax(bad)), got.flat[int(np.argmax(bad))], ref.flat[int(np.argmax(bad))], bar.flat[int(np.argmax(bad))])


def _sum_calls(c, dev):
    """(name, mode, call -> tuple of [C] results, reference operands) of every reduction entry point."""
    y, g, mean, pilot, invstd = (dev[k] for k in ("y", "g", "mean", "pilot", "invstd"))
    calls = [("bn_colsum(y)", "sum", lambda: (K.bn_colsum(y),), dict(y=c["y"])),
             ("bn_colsum(y, mean)", "var", lambda: (K.bn_colsum(y, mean),), dict(y=c["y"], vec=c["mean"])),
             ("bn_colsum2(y, pilot)", "pilot", lambda: K.bn_colsum2(y, pilot), dict(y=c["y"], vec=c["pilot"])),
             ("bn_bwd_colsums", "bwd", lambda: K.bn_bwd_colsums(g, y, mean, invstd), dict(y=c["y"], vec=c["mean"], g=c["g"], invstd=c["invstd"]))]
    if c["C"] % 16 == 0:
        bits = _d(R.pack_bits(c["keep"]))
        calls.append(("bn_bwd_colsums(bits)", "bwd", lambda: K.bn_bwd_colsums(g, y, mean, invstd, bits),
                      dict(y=c["y"], vec=c["mean"], g=c["g"], invstd=c["invstd"], keep=c["keep"])))
    return calls


# ------------------------------------------------------------------------------------------------ 1. the sums, per channel
@pytest.mark.parametrize("C,M,variant", BN_CASES, ids=[_ids(v) for v in BN_CASES])
def test_sums_per_channel_within_the_derived_bar(C, M, variant):
    c = _case(C, M, variant)
    dev = {k: _d(v) for k, v in c.items() if torch.is_tensor(v) and k != "keep"}
    d = R.depth(R.plan(M, C))
    for name, mode, call, ops in _sum_calls(c, dev):
        got, again = call(), call()                       # the wrappers allocate fresh outputs: two independent results
        for a, b in zip(got, again):
            assert torch.equal(a, b), name + ": not bitwise reproducible"
        for i, (t, (ref, bar)) in enumerate(zip(got, R.reference(mode, d, **ops))):
            _within("%s[%d]" % (name, i), t, ref, bar)


# ------------------------------------------------------------------------------------------------ 2. exact integers
@pytest.mark.parametrize("C,M", R.bn_shapes(), ids=["c%d_m%d" % v for v in R.bn_shapes()])
def test_sums_of_integer_data_are_exact(C, M):
    """Every partial sum is an integer multiple of one power of two per channel below 2^24 units (tests/_bn_ref.py make_int_case): exact in any order, so a
    dropped or doubled row shows at every M, also where the rounding bar is wider than one element."""
    ic = _icase(C, M)
    c = dict(ic, pilot=ic["mean"])
    dev = {k: _d(v) for k, v in c.items() if torch.is_tensor(v) and k != "keep"}
    for name, mode, call, ops in _sum_calls(c, dev):
        for i, (t, t64) in enumerate(zip(call(), R.terms(mode, np.float64, **ops))):
            assert torch.equal(t.double().cpu(), torch.from_numpy(t64.sum(0))), "%s[%d]" % (name, i)


# ------------------------------------------------------------------------------------------------ 3. bn_apply, all eight instances, per element
@pytest.mark.parametrize("C,M,variant", BN_CASES, ids=[_ids(v) for v in BN_CASES])
def test_apply_per_element_every_instance(C, M, variant):
    c = _case(C, M, variant)
    scale = (c["gamma"] * c["invstd"])                    # fp32 product on the host: the vector the kernel is handed (the reference reads the same)
    y, res, mean, sc, beta = (_d(t) for t in (c["y"], c["res"], c["mean"], scale, c["beta"]))
    for relu in (False, True):
        for use_res in (False, True):
            ref, bar = R.apply_reference(c["y"], c["mean"], scale, c["beta"], c["res"] if use_res else None, relu)
            for want_mask in ((False, True) if C % 16 == 0 else (False,)):
                out = K.bn_apply(y, mean, sc, beta, res=res if use_res else None, relu=relu, want_mask=want_mask)
                if want_mask:
                    out, bits = out
                    assert torch.equal(R.unpack_bits(bits, C), out.float().view(M, C) > 0), "sign bits != (out > 0)"
                _within("bn_apply relu=%d res=%d bits=%d" % (relu, use_res, want_mask), out, ref, bar)


# ------------------------------------------------------------------------------------------------ 4. bn_bwd_apply, per element
@pytest.mark.parametrize("C,M,variant", BN_CASES, ids=[_ids(v) for v in BN_CASES])
def test_backward_apply_per_element(C, M, variant):
    c = _case(C, M, variant)
    g, y, mean, invstd, gamma = (_d(c[k]) for k in ("g", "y", "mean", "invstd", "gamma"))
    for keep in ((None, c["keep"]) if C % 16 == 0 else (None,)):
        # the sums handed to the kernel: the float64 sums rounded to fp32 (their own error is checked above, not here)
        dbeta, dgamma = (torch.from_numpy(t.sum(0)).float() for t in R.terms("bwd", np.float64, c["y"], c["mean"], c["g"], c["invstd"], keep))
        ref, bar = R.bwd_apply_reference(c["g"], c["y"], c["mean"], c["invstd"], c["gamma"], dbeta, dgamma, M, keep)
        dy = K.bn_bwd_apply(g, y, mean, invstd, gamma, _d(dbeta), _d(dgamma), M, None if keep is None else _d(R.pack_bits(keep)))
        _within("bn_bwd_apply bits=%d" % (keep is not None), dy, ref, bar)


# ------------------------------------------------------------------------------------------------ 5. bn_finalize, per channel
def _bn_module(c, track):
    bn = torch.nn.BatchNorm2d(c["C"], track_running_stats=track).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        if track:
            bn.running_mean.copy_(c["mean"])
            bn.running_var.copy_(torch.from_numpy(R.channel_scale(c["C"]) ** 2).float())
    return bn


def _check_finalize(c, s1, s2, count, track, tag):
    bn = _bn_module(c, track)
    rm0, rv0 = (bn.running_mean.clone(), bn.running_var.clone()) if track else (None, None)
    fin = K.bn_finalize(_d(s1), _d(s2), _d(c["pilot"]), count, bn)
    r = R.finalize_reference(s1, s2, c["pilot"], count, c["gamma"], c["beta"], bn.eps, bn.momentum, rm0, rv0)
    # bn_finalize_channel (batchnorm.hip 208-224) works in double and rounds once: mean, invstd within 2^-23 |ref|; scale = gamma * invstd is one more fp32
    # product: 3 * 2^-24 |ref|
    _within(tag + " mean", fin[0], r["mean"], 2 * R.U32 * np.abs(r["mean"]))
    _within(tag + " invstd", fin[1], r["invstd"], 2 * R.U32 * np.abs(r["invstd"]))
    _within(tag + " scale", fin[2], r["scale"], 3 * R.U32 * np.abs(r["scale"]))
    # shift = beta - (float)mean * scale (batchnorm.hip 214-218) carries five fp32 roundings - of (float)mean, of invstd, of gamma * invstd, of the product and of
    # the difference - each at most 2^-24 of a quantity no larger than |beta| + |mean scale|; one more unit for the second-order terms:
    # 6 * 2^-24 (|beta| + |mean scale|) against float64 throughout.  (The 2^-23 the issue names covers two of the five; no correct kernel keeps it in every channel.)
    _within(tag + " shift", fin[3], r["shift"], 6 * R.U32 * r["shift_terms"])
    # ... and 2^-23 does hold for the last two roundings alone: against beta - mean * scale from the fp32 mean and scale this call returned (pinned just above)
    m_f, sc_f = fin[0].double().cpu().numpy(), fin[2].double().cpu().numpy()
    beta = c["beta"].double().numpy()
    _within(tag + " shift from mean, scale", fin[3], beta - m_f * sc_f, 2 * R.U32 * (np.abs(beta) + np.abs(m_f * sc_f)))
    if track:
        _within(tag + " running_mean", bn.running_mean, r["running_mean"], 2 * R.U32 * np.abs(r["running_mean"]))
        _within(tag + " running_var", bn.running_var, r["running_var"], 2 * R.U32 * np.abs(r["running_var"]))
        assert int(bn.num_batches_tracked) == 1
    return fin


@pytest.mark.parametrize("C,M,variant", BN_CASES, ids=[_ids(v) for v in BN_CASES])
def test_finalize_per_channel_on_the_kernels_own_sums(C, M, variant):
    c = _case(C, M, variant)
    s1, s2 = (t.cpu().clone() for t in K.bn_colsum2(_d(c["y"]), _d(c["pilot"])))
    # count = M (M = 1: the `count > 1` branch of the unbiased factor), and two ranks with the same data: sums and count double (exactly)
    for count, mult in ((M, 1.0), (2 * M, 2.0)):
        for track in (True, False):
            fin = _check_finalize(c, s1 * mult, s2 * mult, count, track, "count=%d track=%d" % (count, track))
    if variant == "const":
        # channel 5 is constant (48) with the pilot 8 below it: s1 = 129 * 8 and s2 = 129 * 64 are exact, the variance is exactly 0 and invstd = 1 / sqrt(eps)
        assert float(s1[5]) == M * 8.0 and float(s2[5]) == M * 64.0
        assert float(fin[1][5]) == float(np.float32(1.0 / np.sqrt(float(np.float32(1e-5)))))
        # and one ulp less in s2: the variance comes out negative (-7.6e-6), `var > 0 ? var : 0` is what keeps invstd at 1 / sqrt(eps)
        s2m = s2.clone()
        s2m[5] = torch.nextafter(s2[5], torch.tensor(0.0))
        fin = _check_finalize(c, s1, s2m, M, True, "negative variance")
        assert float(fin[1][5]) == float(np.float32(1.0 / np.sqrt(float(np.float32(1e-5)))))


# ------------------------------------------------------------------------------------------------ epilogue statistics of mi_conv_gemm_stats
STATS_ROWS = [
    (2, 33, 29, 64, 64, 1, 1, 1),          # the three small rows of test_conv_epilogue_statistics_equal_a_pass_over_the_output
    (2, 33, 29, 64, 256, 3, 1, 2),
    (2, 41, 37, 256, 128, 1, 2, 1),
    (2, 33, 29, 64, 48, 1, 1, 1),          # N = 48: the last 32-channel group of bn_reduce_stage1_kernel is half empty
    (5, 29, 113, 64, 64, 1, 1, 1),         # M = 16 385 = 128 * 128 + 1: 129 row tiles of 128 rows, 258 partial rows > BN_RED_ROWS = 256: nsplit = 2 (16 384: 256, nsplit 1)
]


@pytest.mark.parametrize("B,H,W,Ca,N,k,stride,dil", STATS_ROWS)
def test_conv_epilogue_statistics_per_channel(B, H, W, Ca, N, k, stride, dil):
    g = torch.Generator().manual_seed(B * H + Ca + N + k)
    pad = dil * (k // 2)
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    M = B * Ho * Wo
    plan = K.conv_gemm_plan((B, H, W, Ca), N, (Ho, Wo), k, stride, pad, dil, 512)
    nparts = 2 * plan.m_tiles                                              # igemm_nt.hip 597 / igemm_pp.hip 744: one partial row per wave row of a tile
    if M == 16385:
        assert nparts == 258 and 2 * K.conv_gemm_plan((1, 128, 128, Ca), N, (128, 128), k, stride, pad, dil, 512).m_tiles == 256
    x = torch.randn(B, H, W, Ca, generator=g).to(torch.bfloat16).to(DEV)
    w = torch.randn(N, Ca, k, k, generator=g) / (Ca * k * k) ** 0.5 * torch.from_numpy(R.channel_scale(N)).float().view(N, 1, 1, 1)
    wp = K.pack_weight_fwd(w.to(DEV))
    want = K.conv_gemm(x, wp, (Ho, Wo), k, stride, pad, dil, K.GATHER_FWD)
    o64 = want.double().cpu().view(M, N)
    pilot = (o64.mean(0) + o64.std(0, unbiased=False) * torch.cos(3.0 * torch.arange(N).double())).float()        # within one sigma of the mean
    got, (s1, s2), _ = K.conv_gemm_stats(x, wp, (Ho, Wo), k, stride, pad, dil, _d(pilot))
    assert torch.equal(got, want)
    again = K.conv_gemm_stats(x, wp, (Ho, Wo), k, stride, pad, dil, _d(pilot))[1]
    assert torch.equal(again[0], s1) and torch.equal(again[1], s2)
    d = R.depth_stats(32 * plan.mt, nparts)
    for i, (t, (ref, bar)) in enumerate(zip((s1, s2), R.reference("pilot", d, want.cpu().view(M, N), vec=pilot))):
        _within("conv_gemm_stats s%d (%s, %d partial rows)" % (i + 1, plan.name, nparts), t, ref, bar)


# ------------------------------------------------------------------------------------------------ csrc/colsum.hip
SENT = -7777.0
COLSUM_CASES = [(1, N, M) for N, M in R.colsum_shapes(R.ASPP_K, 1)] + [(8, N, M) for N, M in R.colsum_shapes(R.BIAS_N, 8)]


def _colsum(vec, x, out, accumulate=False):
    M, N = x.shape
    return K.aspp_bias_grad(x.view(1, 1, M, N), out, accumulate) if vec == 1 else K.bias_grad_bf16(x.view(1, 1, M, N), out, accumulate)


@pytest.mark.parametrize("vec,N,M", COLSUM_CASES, ids=["%s_n%d_m%d" % ("aspp" if v == 1 else "bf16", n, m) for v, n, m in COLSUM_CASES])
def test_bias_gradient_column_sums_per_channel(vec, N, M):
    rep = 4 if vec == 1 else 1                            # mi_aspp_bias_grad writes the sum to the 4 ASPP branches
    d = R.depth(R.colsum_plan(M, N, vec))
    x = R.make_colsum_case(N, M, vec == 8)
    xi = R.make_colsum_int_case(N, M, vec == 8)
    xd, xid = _d(x), _d(xi)
    buf = torch.full((rep * N + 128,), SENT, device=DEV)
    out = buf[64:64 + rep * N]
    _colsum(vec, xd, out)
    plain = out.clone()
    assert bool((buf[:64] == SENT).all()) and bool((buf[64 + rep * N:] == SENT).all()), "written outside [0, %d)" % (rep * N)
    (ref, bar), = R.reference("colsum", d, x)
    for r in range(rep):
        assert torch.equal(plain[r * N:(r + 1) * N], plain[:N]), "replica %d differs" % r
        _within("colsum replica %d" % r, plain[r * N:(r + 1) * N], ref, bar)
    _colsum(vec, xd, out)
    assert torch.equal(out, plain), "not bitwise reproducible"
    # accumulate: db_before + plain result, rounded once (colsum.hip 63)
    before = (torch.randn(rep * N, generator=torch.Generator().manual_seed(N + M)) * torch.from_numpy(R.channel_scale(N)).float().repeat(rep))
    out.copy_(before)
    _colsum(vec, xd, out, accumulate=True)
    assert torch.equal(out.cpu(), before + plain.cpu())
    assert bool((buf[:64] == SENT).all()) and bool((buf[64 + rep * N:] == SENT).all())
    # integers: exact in any order
    _colsum(vec, xid, out)
    exact = torch.from_numpy(R.terms("colsum", np.float64, xi)[0].sum(0))
    assert torch.equal(out.double().cpu(), exact.repeat(rep))
