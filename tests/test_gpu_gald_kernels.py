"""GPU parity of the kernels only GALD (HarDNet-68 + GCPA) trains with, each called through the C-ABI and compared with a plain float64 torch
computation on the SAME bf16-rounded operands: the criss-cross attention core (csrc/gald.hip: gcca_fwd / gcca_bwd_a / gcca_bwd_b), the sigmoid
gate of the local attention module (ggate), HarDNet's max pools with their one-byte winner index and the cross-entropy of the deep-supervision
heads on NHWC fp32 logits (csrc/gnet.hip: gmaxpool, gce).  The shapes are picked for the branches the kernels take: the product's Cq = 32 and
C = 256, more than 64 and more than 256 attention candidates, the scalar datt path (C % 8 != 0, a misaligned view), the VEC 8 / 2 / 1 pools,
grid-stride second trips, and ties.

Bars come from each kernel's rounding model.  A bf16 output of an fp32 chain of n roundings is within one bf16 ulp of the exact value plus
2 * n * 2^-24 times the sum of the absolute values of its terms (the floor of _close_bf16, taken at the tensor's largest such sum; 2: slack on
the first-order model).  Every check prints its worst error next to its bar.  The restatement of the attention in float64 is pinned to the
fixture-checked oracle (oracle/ref_gald.py CrissCross) by the one CPU test of this file."""
import pytest
import torch
import torch.nn.functional as F

from _parity import _close_bf16, _embed, _nhwc, _rand

gpu = pytest.mark.gpu
U = 2.0 ** -24          # fp32 unit roundoff


@pytest.fixture(scope="module")
def gk():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import gk as g
    return g


def _chain(got, ref, absum, n, what):
    """bf16 `got` against the float64 `ref` of an fp32 chain of n roundings whose terms have absolute sums `absum` (same shape as ref)."""
    ref = ref.double()
    rmax = float(ref.abs().max())
    floor = 2 * n * U * float(absum.max()) / max(rmax, 1e-300)
    tol = 2.0 ** -8 * ref.abs() + floor * rmax
    err = (got.double().cpu() - ref).abs()
    print("%s: worst |err| / bar %.3f (worst |err| %.2e, floor %.2e of max |ref| %.2e, n = %d)" % (what, float((err / tol.clamp_min(1e-300)).max()),
                                                                                                 float(err.max()), floor, rmax, n))
    _close_bf16(got, ref, what, floor=floor)


def _within(got, ref, tol, what):
    err = (got.double().cpu() - ref.double()).abs()
    print("%s: worst |err| / bar %.3f (worst |err| %.2e)" % (what, float((err / tol.clamp_min(1e-300)).max()), float(err.max())))
    bad = err > tol
    assert not bad.any(), "%s: %d of %d outside the bar, worst %.3e" % (what, int(bad.sum()), bad.numel(), float(err.max()))


# ------------------------------------------------------------------------------------------------ criss-cross attention core
# Candidates of pixel (b, h, w): j < H the column (b, j, w), j = H + v the row (b, h, v); the column's own position j == h is masked.
def _affinity(a, b):
    """sum_c a[pixel, c] b[candidate j, c] for every candidate: [B,H,W,H+W] (no mask)."""
    return torch.cat([torch.einsum("bhwc,bgwc->bhwg", a, b), torch.einsum("bhwc,bhvc->bhwv", a, b)], 3)


def _gather(att, x):
    """sum_j att[pixel, j] x[candidate j]"""
    H = x.shape[1]
    return torch.einsum("bhwg,bgwc->bhwc", att[..., :H], x) + torch.einsum("bhwv,bhvc->bhwc", att[..., H:], x)


def _scatter(att, y):
    """the transpose of _gather: sum over the pixels p that have me as candidate j of att_p[j] y_p"""
    H = y.shape[1]
    return torch.einsum("bhwg,bhwc->bgwc", att[..., :H], y) + torch.einsum("bhwv,bhwc->bhvc", att[..., H:], y)


def _cca_ref(q, k, v):
    """oracle/ref_gald.py CrissCross's attention core (einsums, the column's own position masked with -inf, ONE softmax over the H + W candidates)
    restated on NHWC tensors: q, k [B,H,W,Cq], v [B,H,W,C] -> (att [B,H,W,H+W], agg [B,H,W,C])."""
    H = q.shape[1]
    e_col = torch.einsum("bhwc,bgwc->bhwg", q, k).masked_fill(torch.eye(H, dtype=torch.bool).view(1, H, 1, H), float("-inf"))
    e_row = torch.einsum("bhwc,bhvc->bhwv", q, k)
    att = torch.softmax(torch.cat([e_col, e_row], 3), 3)
    return att, _gather(att, v)


def test_criss_cross_restatement_equals_the_oracle_module():
    """The float64 restatement the GPU tests use is the oracle's module: q, k, v from CrissCross's own 1x1 convs, gamma * agg + x == CrissCross(x)."""
    from oracle import ref_gald as rg
    g = torch.Generator().manual_seed(5)
    m = rg.CrissCross(32).double()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.5)
        m.gamma.fill_(0.7)
    x = torch.randn((2, 32, 5, 7), generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = m(x)
        q, k, v = (_nhwc(c(x)) for c in (m.query_conv, m.key_conv, m.value_conv))
        att, agg = _cca_ref(q, k, v)
        got = m.gamma * agg.permute(0, 3, 1, 2) + x
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    assert float((got - x).abs().max()) > 0.1                                          # the attention term is really there


CCA_CASES = [
    # B, H, W, Cq, C, views
    (2, 22, 40, 32, 256, False),   # the product at 720x1280: 62 candidates, cw = 32 (8 dq groups), C + Cq = 288 > 256 in bwd_b
    (1, 32, 32, 32, 256, False),   # H + W = 64: exactly one datt chunk
    (1, 32, 33, 20, 40, False),    # 65 candidates: the second datt chunk holds one; Cq no power of two
    (1, 40, 60, 8, 36, False),     # C % 8 != 0: the scalar datt path, two chunks
    (1, 64, 200, 8, 16, False),    # H + W = 264 > 256: two candidates per thread in the softmax and in de; five datt chunks
    (1, 7, 9, 260, 264, False),    # Cq > 256 (two dq passes of cw = 256), C > 256
    (2, 1, 9, 8, 16, False),       # H = 1: the column is only the masked position
    (2, 7, 1, 8, 16, False),       # W = 1
    (1, 1, 1, 8, 16, False),       # one pixel: att = [0, 1]
    (2, 9, 11, 16, 40, True),      # channel slices; v 8 bytes off 16-byte alignment (ld % 8 == 0, C % 8 == 0): scalar datt for the alignment reason
]


@gpu
@pytest.mark.parametrize("case", CCA_CASES)
def test_criss_cross_attention_core_against_float64(gk, case):
    B, H, W, Cq, C, views = case
    J = H + W
    s = 1.3 * Cq ** -0.25                                  # logits of standard deviation ~1.7
    q, k = _nhwc(_rand((B, Cq, H, W), 11 + Cq, s)), _nhwc(_rand((B, Cq, H, W), 12 + Cq, s))
    v, dagg = _nhwc(_rand((B, C, H, W), 13 + C)), _nhwc(_rand((B, C, H, W), 14 + C))
    if views:
        qk_big = torch.full((B, H, W, 48), 7.0, dtype=torch.bfloat16, device="cuda")
        qk_big[..., 4:4 + Cq], qk_big[..., 24:24 + Cq] = q.cuda(), k.cuda()
        qv, kv = qk_big[..., 4:4 + Cq], qk_big[..., 24:24 + Cq]
        _, vv = _embed(v.cuda(), 56, 4)                    # 8-byte offset, 112-byte rows
        _, gv = _embed(dagg.cuda(), 48, 8)                 # 16-byte aligned
        assert vv.data_ptr() % 16 == 8 and C % 8 == 0
    else:
        qv, kv, vv, gv = q.cuda(), k.cuda(), v.cuda(), dagg.cuda()
    agg, att = gk.gcca_fwd(qv, kv, vv)
    dq, dk, dv = gk.gcca_bwd(qv, kv, vv, att, gv)
    dq2, dk2, dv2 = gk.gcca_bwd(qv, kv, vv, att, gv)
    torch.cuda.synchronize()
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2), "the backward is not bit-reproducible"

    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    att_r, agg_r = _cca_ref(qd, kd, vd)
    agg_r.backward(dagg.double())
    att_r = att_r.detach()
    # rounding model.  Logits: fp32 sums of Cq exact bf16 products, |error| <= Cq u A (A = the largest sum |q_c k_c|); the softmax doubles it for
    # the difference to the maximum and again for the normalisation, the fast exponential adds |arg| u <= 2 A u and an ulp, the sum J u.
    A = float(_affinity(q.double().abs(), k.double().abs()).max())
    n_att = int(4 * Cq * A + 4 * A + J + 8)
    a = att.double().cpu()
    err = (a - att_r).abs()
    tol = 2 * n_att * U * att_r
    print("att: worst |err| / bar %.3f (worst |err| %.2e, n = %d)" % (float((err / tol.clamp_min(1e-300)).max()), float(err.max()), n_att))
    assert not bool((err > tol).any()), "att: %d of %d outside the bar" % (int((err > tol).sum()), err.numel())
    rs = (a.sum(3) - 1).abs()
    print("att row sums: worst |sum - 1| %.2e, bar %.2e" % (float(rs.max()), 2 * (J + 3) * U))
    assert float(rs.max()) <= 2 * (J + 3) * U
    own = torch.arange(H).view(1, H, 1, 1).expand(B, H, W, 1)
    assert bool((torch.gather(a, 3, own) == 0).all()), "the column's own position is not masked to exactly 0"
    _chain(agg, agg_r.detach(), _gather(att_r, v.double().abs()), J + 1 + n_att, "agg %s" % (case,))
    # backward: datt (C terms), the dot sum_j att datt (J terms), de = att (datt - dot), then the J-term sums of dq / dk; dv: J terms of att dagg
    dabs = _affinity(dagg.double().abs(), v.double().abs())
    de_abs = att_r * (dabs + (att_r * dabs).sum(3, keepdim=True))
    n_b = 2 * J + C + n_att + 2
    _chain(dq, qd.grad, _gather(de_abs, k.double().abs()), n_b, "dq %s" % (case,))
    _chain(dk, kd.grad, _scatter(de_abs, q.double().abs()), n_b, "dk %s" % (case,))
    _chain(dv, vd.grad, _scatter(att_r, dagg.double().abs()), J + 1 + n_att, "dv %s" % (case,))


# ------------------------------------------------------------------------------------------------ max pools
def _pool_input(shape, seed):
    """half small integers, half ReLU6-style clamped values (0 and 6 everywhere): most windows tie"""
    g = torch.Generator().manual_seed(seed)
    ints = torch.randint(-3, 4, shape, generator=g).float()
    clamped = (torch.randn(shape, generator=g) * 4).clamp(0, 6)
    return torch.where(torch.rand(shape, generator=g) < 0.5, ints, clamped).to(torch.bfloat16)


def _dyadic(shape, seed):
    """multiples of 1/4 in [-2, 2): a sum of up to four is exact in bf16"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 8, shape, generator=g).float() / 4).to(torch.bfloat16)


def _taps(ind, H, W, k, s, p):
    """torch's return_indices (flat input position) -> the tap number ky * k + kx of the kernel's one-byte index"""
    Ho, Wo = ind.shape[2], ind.shape[3]
    oh, ow = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    return (ind // W - (oh * s - p)) * k + (ind % W - (ow * s - p))


def _check_max_pool(gk, x, k, s, p, ld, off, seed, what):
    B, C, H, W = x.shape
    xd = x.double().requires_grad_(True)
    ref, ind = F.max_pool2d(xd, k, s, p, return_indices=True)
    dout = _dyadic(tuple(ref.shape), seed)
    ref.backward(dout.double())
    _, xv = _embed(_nhwc(x).cuda(), ld, off)               # the sentinel (7) beats every value: a read outside the slice would win
    out, idx = gk.gmaxpool(xv, k, s, p)
    _, dov = _embed(_nhwc(dout).cuda(), ld, off)
    dbig = torch.full((B, H, W, ld), 5.0, dtype=torch.bfloat16, device="cuda")
    dx = gk.gmaxpool_bwd(dov, idx, (H, W), k, s, p, dx=dbig[..., off:off + C])
    torch.cuda.synchronize()
    o = out.permute(0, 3, 1, 2).double().cpu()
    print("%s: forward %d of %d differ, idx %d differ, dx %d differ (bar: 0)" % (what, int((o != ref.detach()).sum()), o.numel(),
                                                                                    int((idx.permute(0, 3, 1, 2).long().cpu() != _taps(ind, H, W, k, s, p)).sum()),
                                                                                    int((dx.permute(0, 3, 1, 2).cpu() != xd.grad.to(torch.bfloat16)).sum())))
    assert torch.equal(o, ref.detach()), what
    assert torch.equal(idx.permute(0, 3, 1, 2).long().cpu(), _taps(ind, H, W, k, s, p)), "%s: winner index is not the first maximum in scan order" % what
    assert torch.equal(dx.permute(0, 3, 1, 2).cpu(), xd.grad.to(torch.bfloat16)), what
    assert bool((dbig[..., :off] == 5.0).all()) and bool((dbig[..., off + C:] == 5.0).all()), "%s: the backward wrote outside its slice" % what


MAXPOOL_CASES = [
    # k, s, p, B, H, W, C, (ld, off): x, dout and dx as channel slices [off, off + C) of ld-wide tensors
    (3, 2, 1, 2, 45, 79, 64, (64, 0)),      # HarDNet's stem pool on odd H and W, VEC 8
    (2, 2, 0, 2, 45, 80, 64, (64, 0)),      # a transition pool on the 45 x 80 map of a 720 x 1280 crop, VEC 8
    (3, 2, 1, 2, 13, 11, 26, (40, 2)),      # 4-byte aligned slice: VEC 2
    (2, 2, 0, 2, 13, 11, 26, (40, 2)),
    (3, 2, 1, 2, 13, 11, 24, (40, 3)),      # C % 8 == 0 at an odd offset: VEC 1
    (2, 2, 0, 1, 15, 9, 13, (13, 0)),       # odd C: VEC 1
]


@gpu
@pytest.mark.parametrize("case", MAXPOOL_CASES)
def test_max_pool_forward_index_and_backward_exact(gk, case):
    """Forward equals F.max_pool2d exactly, the winner index equals torch's return_indices as a tap number (torch keeps the FIRST maximum in scan
    order, which matters on ReLU6 outputs tied at 0 and 6), and the backward of dyadic gradients equals torch's bit for bit."""
    k, s, p, B, H, W, C, (ld, off) = case
    _check_max_pool(gk, _pool_input((B, C, H, W), 30 + C + H), k, s, p, ld, off, 31 + C, "maxpool %s" % (case,))


@gpu
def test_max_pool_grid_stride_second_trip(gk):
    """C = 1 at 4 x 2101 x 2101: 4 410 000 output and 17.7 M input elements, more than the 16 384 x 256 threads of a capped grid in both
    directions (4 images: one 2101 x 2101 map pools to 1 102 500 outputs, too few for the forward's second trip)."""
    _check_max_pool(gk, _pool_input((4, 1, 2101, 2101), 41), 2, 2, 0, 1, 0, 42, "maxpool 4x2101x2101x1")


# ------------------------------------------------------------------------------------------------ sigmoid gate
@gpu
@pytest.mark.parametrize("B,H,W,C,views", [(2, 9, 13, 32, False), (2, 9, 13, 40, True), (1, 260, 256, 64, False)])
def test_sigmoid_gate_forward_backward(gk, B, H, W, C, views):
    """out = x + x * sigmoid(g); dx = dout * (1 + s), dg = dout * x * s * (1 - s), with saturated gates (|g| = 20, 90) and channel-slice views; the
    last case has 4.26 M elements (a second grid-stride trip).  Bar: one bf16 ulp plus the fp32 error of s = 1 / (1 + exp(-g)) (|g| u from the
    exponent's argument, a few ulps for exp, add and divide) carried through the products."""
    x, g, dout = _rand((B, H, W, C), 50 + C, 2.0), _rand((B, H, W, C), 51 + C, 4.0), _rand((B, H, W, C), 52 + C)
    sat = torch.tensor([20.0, -20.0, 90.0, -90.0], dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(53)
    pick = torch.rand(g.shape, generator=gen) < 0.15
    g = torch.where(pick, sat[torch.randint(0, 4, g.shape, generator=gen)], g)
    if views:
        (_, xv), (_, gv), (_, dv) = _embed(x.cuda(), 48, 4), _embed(g.cuda(), 56, 8), _embed(dout.cuda(), 44, 2)
    else:
        xv, gv, dv = x.cuda(), g.cuda(), dout.cuda()
    out = gk.ggate(xv, gv)
    dx, dg = gk.ggate_bwd(xv, gv, dv)
    torch.cuda.synchronize()
    xd, gd, dd = x.double(), g.double(), dout.double()
    sg = torch.sigmoid(gd)
    e = 2 * U * (8 + 2 * gd.abs())
    ref = xd + xd * sg
    _within(out, ref, 2.0 ** -8 * ref.abs() + e * xd.abs(), "gate out %s" % ((B, H, W, C, views),))
    ref = dd * (1 + sg)
    _within(dx, ref, 2.0 ** -8 * ref.abs() + e * dd.abs(), "gate dx %s" % ((B, H, W, C, views),))
    ref = dd * xd * sg * (1 - sg)
    _within(dg, ref, 2.0 ** -8 * ref.abs() + 2 * e * (dd * xd).abs(), "gate dg %s" % ((B, H, W, C, views),))


# ------------------------------------------------------------------------------------------------ cross-entropy on NHWC fp32 logits
def _ce_case(K, ld, mag, seed):
    """fp32 logits [B,H,W,K] as a channel slice of an ld-wide tensor; labels with ~10 % ignored (255) and a few out of range (K, -1, 33)"""
    B, H, W = 2, 37, 61
    g = torch.Generator().manual_seed(seed)
    z = (torch.rand((B, H, W, K), generator=g) * 2 - 1) * mag
    lab = torch.randint(0, K, (B, H, W), generator=g)
    lab[torch.rand((B, H, W), generator=g) < 0.1] = 255
    lab[0, 3, 5:9] = K
    lab[1, 20, 7] = -1
    lab[1, 36, 60] = 33
    big = torch.full((B, H, W, ld), 7.0, device="cuda")
    big[..., ld - K:] = z.cuda()
    return z, lab, big[..., ld - K:]


@gpu
@pytest.mark.parametrize("K,ld,mag,grad_scale", [(19, 19, 4.0, 1.0), (19, 24, 80.0, 0.37), (1, 1, 4.0, 1.0), (32, 40, 4.0, 2.5), (32, 32, 80.0, 1.0)])
def test_nhwc_cross_entropy_against_torch(gk, K, ld, mag, grad_scale):
    """gk.gce (the GALD trainer's criterion) against F.cross_entropy(ignore_index=255) in float64: 4 514 rows (four 1 024-row blocks and a ragged
    tail), logits views with ld > K, magnitude 80, ignored pixels, grad_scale != 1.  Out-of-range labels are counted in loss_out[2] and left out of
    the loss and its gradient (torch would raise; the reference maps them to ignore_index).  want_grad=False gives the same loss bits.  Bars: those
    of the DeepLab CE tests - loss 2e-6 relative, gradient 2e-5 of its largest element."""
    z, lab, zv = _ce_case(K, ld, mag, 60 + K)
    bad = (lab != 255) & ((lab < 0) | (lab >= K))
    labd = lab.cuda()
    out, d = gk.gce(zv, labd, grad_scale=grad_scale)
    out2, d2 = gk.gce(zv, labd, want_grad=False)
    torch.cuda.synchronize()
    lr = torch.where(bad, torch.full_like(lab, 255), lab)
    zd = z.double().permute(0, 3, 1, 2).requires_grad_(True)
    loss = F.cross_entropy(zd, lr, ignore_index=255)
    (loss * grad_scale).backward()
    o = out.double().cpu()
    le = abs(float(o[0]) - float(loss))
    print("ce K=%d ld=%d mag=%g: loss |err| %.2e, bar %.2e" % (K, ld, mag, le, 2e-6 * abs(float(loss))))
    assert le <= 2e-6 * abs(float(loss))
    assert int(o[1]) == int((lr != 255).sum()) and int(o[2]) == int(bad.sum()) == 6
    gr = zd.grad.permute(0, 2, 3, 1)
    ge = float((d.double().cpu() - gr).abs().max())
    gmax = float(gr.abs().max())
    print("ce K=%d ld=%d mag=%g: gradient |err| %.2e, bar %.2e" % (K, ld, mag, ge, 2e-5 * gmax))
    assert ge <= 2e-5 * gmax
    assert bool((d.cpu()[lr == 255] == 0).all()), "ignored or out-of-range pixels got a gradient"
    assert d2 is None and torch.equal(out2[:3], out[:3])


@gpu
def test_nhwc_cross_entropy_all_ignored_and_refusals(gk):
    """All pixels ignored: the kernel returns loss NaN (mean over no pixel, as torch does), a valid count of 0 and an all-zero gradient.  K = 33 is
    refused (the kernel keeps one pixel's logits in registers for K <= 32)."""
    from rnd_semantic_segmentation_amd._lib import MiError
    z, lab, zv = _ce_case(19, 19, 4.0, 70)
    out, d = gk.gce(zv, torch.full_like(lab, 255).cuda(), grad_scale=3.0)
    torch.cuda.synchronize()
    assert torch.isnan(out[0]) and float(out[1]) == 0 and float(out[2]) == 0
    assert bool((d == 0).all())
    with pytest.raises(MiError):
        gk.gce(torch.zeros((1, 2, 2, 33), device="cuda"), torch.zeros((1, 2, 2), dtype=torch.int64, device="cuda"))
