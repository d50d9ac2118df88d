"""The references and bars of tests/_bn_ref.py bite before a GPU is involved: the kernels' summation order, emulated in numpy float32 on the very data
tests/test_gpu_bn_parity.py uses, lies INSIDE the derived bar in every case and channel; the same emulation with a row dropped, the last row counted twice or
two 8-channel slots swapped lies OUTSIDE it (or, where M is so large that the rounding bar is wider than one element, differs on the exact-integer data,
which that case's torch.equal check then catches)."""
import numpy as np
import pytest

import _bn_ref as R

F32 = np.float32


def test_plan_reproduces_the_numbers_of_the_kernel_comments():
    # bn_plan at layer-3's M = 8 * 97 * 97 = 75 272 pixels, C = 256: 32 slots, 8 row lanes, blocks of ceil(75272 / 256) = 295 -> 296 rows
    p = R.plan(75272, 256)
    assert (p.slots, p.cp, p.L, p.rows_per_block, p.nblocks) == (32, 32, 8, 296, 255)
    assert R.depth(p) == 37 + 8 + 8 + 32
    assert [R.plan(1, C).L for C in R.BN_CHANNELS] == [256, 64, 32, 32, 4, 1, 1]
    assert [R.plan(1, C).cp - R.plan(1, C).slots for C in R.BN_CHANNELS] == [0, 1, 2, 0, 31, 125, 0]          # idle slots per row
    # the edges the shape list is there for
    for C in R.BN_CHANNELS:
        L = R.plan(1, C).L
        assert R.plan(256 * L, C)[3:] == (L, 256) and R.plan(256 * L + 1, C)[3:] == (2 * L, 129)              # the last block of 256L + 1 holds one row
        assert (256 * L + 1) - 128 * 2 * L == 1
        assert R.plan(33 * 7 * L + 5, C).nblocks % 32 != 0
    assert max(M for _, M in R.bn_shapes()) == 2048 * 256 and len(R.bn_shapes()) == len(set(R.bn_shapes()))
    # bn_apply_kernel / bn_bwd_apply_kernel: a thread per 8 channels, 256 per workgroup - every C has cases whose last workgroup is partly idle, and cases with
    # more than one workgroup.  (C = 2048 cannot: its 256 slots make n8 = 256 M a whole number of workgroups at every M.)
    for C in R.BN_CHANNELS:
        n8 = [M * C // 8 for c, M in R.bn_shapes() if c == C]
        assert C == 2048 or (any(n % 256 for n in n8) and any(n > 256 and n % 256 for n in n8)), C
        assert any(n > 256 for n in n8)
    # colsum.hip: a block is at least 8 L rows, at most 512 blocks, the block height is no multiple of L above the cap
    assert R.colsum_plan(8 * 256, 1, 1)[2:] == (256, 2048, 1) and R.colsum_plan(8 * 256 + 1, 1, 1)[2:] == (256, 2048, 2)
    assert R.colsum_plan(512 * 8 * 8 + 1, 19, 1)[2:] == (8, 65, 505)
    assert R.colsum_plan(4097, 2048, 8) == R.Plan(256, 256, 1, 9, 456)
    assert R.depth_stats(128, 258) == 128 + 8 + 32 + 2


def _reductions(case):
    """(name, mode, operands) of every sum the GPU test checks on a standard case."""
    y, g, mean, pilot, invstd, keep = (case[k] for k in ("y", "g", "mean", "pilot", "invstd", "keep"))
    out = [("colsum", "sum", dict(y=y)), ("colsum_mean", "var", dict(y=y, vec=mean)), ("colsum2", "pilot", dict(y=y, vec=pilot)),
           ("bwd", "bwd", dict(y=y, vec=mean, g=g, invstd=invstd))]
    if case["C"] % 16 == 0:
        out.append(("bwd_bits", "bwd", dict(y=y, vec=mean, g=g, invstd=invstd, keep=keep)))
    return out


def _outside(got, ref, bar):
    return bool((np.abs(got.astype(np.float64) - ref) > bar).any())


@pytest.mark.parametrize("C,M", R.bn_shapes())
def test_emulated_kernel_order_is_inside_the_bar_and_wrong_sums_are_outside(C, M):
    p = R.plan(M, C)
    d = R.depth(p)
    case = R.make_bn_case(C, M)
    small = M * d * R.U32 < 1.0 / 8            # the rounding bar is narrower than (about a quarter of) one average element
    icase = R.make_int_case(C, M)
    for name, mode, ops in _reductions(case):
        refs = R.reference(mode, d, **ops)
        t32 = R.terms(mode, F32, **ops)
        for (ref, bar), t in zip(refs, t32):
            got = R.emulate(t, p)
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bar).all(), (name, int(np.argmax(err - bar)), float((err / np.maximum(bar, 1e-300)).max()))
        # a wrong sum must fail the case: some output of the reduction leaves its bar in some channel
        wrong = {"dropped row": dict(drop=M // 2), "last row twice": dict(twice_last=True)}
        if p.slots > 1:
            wrong["swapped slots"] = dict(swap=(0, p.slots - 1))
        for what, kw in wrong.items():
            if small or what == "swapped slots":
                assert any(_outside(R.emulate(t, p, **kw), ref, bar) for (ref, bar), t in zip(refs, t32)), (name, what)
            else:       # large M: the exact-integer check of the same case is the one that must see it
                iops = dict(y=icase["y"]) if mode == "sum" else dict(y=icase["y"], vec=icase["mean"])
                if mode == "bwd":
                    iops.update(g=icase["g"], invstd=icase["invstd"], keep=icase["keep"] if "keep" in ops else None)
                exact = [t.sum(0) for t in R.terms(mode, np.float64, **iops)]
                it32 = R.terms(mode, F32, **iops)
                assert all(np.array_equal(R.emulate(t, p).astype(np.float64), e) for t, e in zip(it32, exact)), (name, "the integer sums are exact")
                assert any(not np.array_equal(R.emulate(t, p, **kw).astype(np.float64), e) for t, e in zip(it32, exact)), (name, what)


def test_the_large_cases_are_the_ones_left_to_the_integer_check():
    large = [(C, M) for C, M in R.bn_shapes() if not M * R.depth(R.plan(M, C)) * R.U32 < 1.0 / 8]
    assert (8, 65537) in large and (8, 4 * 256 + 1) not in large and (2048, 2048) not in large and all(M > 2 ** 13 for _, M in large)
    # the four-row trip (batchnorm.hip 72) runs in exactly the shapes added for it
    trip = [(C, M) for C, M in R.bn_shapes() if R.plan(M, C).rows_per_block >= 4 * R.plan(M, C).L]
    assert trip == [(C, f * R.plan(1, C).L + e) for C in R.BN_CHANNELS for f, e in ((1024, 0), (1024, 1), (1792, 0), (2048, 0))]
    assert [R.plan(M, C).rows_per_block // R.plan(M, C).L for C, M in trip] == [4, 5, 7, 8] * len(R.BN_CHANNELS)


@pytest.mark.parametrize("C,M", R.bn_shapes())
def test_integer_data_sums_exactly_in_the_kernel_order(C, M):
    p = R.plan(M, C)
    ic = R.make_int_case(C, M)
    for mode, ops in (("sum", dict(y=ic["y"])), ("var", dict(y=ic["y"], vec=ic["mean"])), ("pilot", dict(y=ic["y"], vec=ic["mean"])),
                      ("bwd", dict(y=ic["y"], vec=ic["mean"], g=ic["g"], invstd=ic["invstd"], keep=ic["keep"]))):
        for t32, t64 in zip(R.terms(mode, F32, **ops), R.terms(mode, np.float64, **ops)):
            assert np.array_equal(R.emulate(t32, p).astype(np.float64), t64.sum(0)), mode


@pytest.mark.parametrize("vec,N,M", [(1, N, M) for N, M in R.colsum_shapes(R.ASPP_K, 1)] + [(8, N, M) for N, M in R.colsum_shapes(R.BIAS_N, 8)])
def test_colsum_order_is_inside_the_bar_and_wrong_sums_are_outside(vec, N, M):
    p = R.colsum_plan(M, N, vec)
    d = R.depth(p)
    x = R.make_colsum_case(N, M, vec == 8)
    (ref, bar), = R.reference("colsum", d, x)
    t, = R.terms("colsum", F32, x)
    assert (np.abs(R.emulate(t, p).astype(np.float64) - ref) <= bar).all()
    xi = R.make_colsum_int_case(N, M, vec == 8)
    ti, = R.terms("colsum", F32, xi)
    exact = R.terms("colsum", np.float64, xi)[0].sum(0)
    assert np.array_equal(R.emulate(ti, p).astype(np.float64), exact)
    for kw in (dict(drop=M // 2), dict(twice_last=True)):
        if M * d * R.U32 < 1.0 / 8:
            assert _outside(R.emulate(t, p, **kw), ref, bar), kw
        else:
            assert not np.array_equal(R.emulate(ti, p, **kw).astype(np.float64), exact), kw


def test_per_element_bars_hold_for_fp32_arithmetic_and_see_a_wrong_slot():
    """bn_apply / bn_bwd_apply in numpy float32, operation by operation as the kernels write them, then one bf16 rounding: inside the per-element bar; with the
    parameters of the neighbouring slot: outside."""
    import torch
    c = R.make_bn_case(64, 129)
    y, g, res = (c[k].float().numpy() for k in ("y", "g", "res"))
    mean, invstd, gamma, beta = (c[k].numpy() for k in ("mean", "invstd", "gamma", "beta"))
    scale = (gamma * invstd).astype(F32)
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).double().numpy()
    for relu in (False, True):
        ref, bar = R.apply_reference(c["y"], mean, scale, beta, c["res"], relu)
        t = ((y - mean) * scale + beta) + res
        t = np.maximum(t, F32(0)) if relu else t
        assert (np.abs(bf(t) - ref) <= bar).all()
        t = ((y - np.roll(mean, 8)) * np.roll(scale, 8) + np.roll(beta, 8)) + res
        assert (np.abs(bf(np.maximum(t, F32(0)) if relu else t) - ref) > bar).any()
    dbeta, dgamma = (t.sum(0).astype(F32) for t in R.terms("bwd", np.float64, c["y"], mean, c["g"], invstd))
    M = 129
    ic = F32(1.0 / M)
    ref, bar = R.bwd_apply_reference(c["g"], c["y"], mean, invstd, gamma, dbeta, dgamma, M)
    dy = lambda mean, invstd, gamma, dbeta, dgamma: gamma * invstd * (g - dbeta * ic - ((y - mean) * invstd) * dgamma * ic)
    assert (np.abs(bf(dy(mean, invstd, gamma, dbeta, dgamma)) - ref) <= bar).all()
    assert (np.abs(bf(dy(*(np.roll(v, 8) for v in (mean, invstd, gamma, dbeta, dgamma)))) - ref) > bar).any()
