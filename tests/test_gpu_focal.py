"""GPU tests of the focal loss in the fused upsample + cross-entropy heads (mi_upsample_ce_focal, csrc/upsample_ce.hip) and the layers above it:
K.upsample_ce_focal against the float64 restatement (tests/_focal_ref.py) and torch's own float64 composition, gamma = 0 against the bytes of
mi_upsample_ce_w / mi_upsample_ce_ex, the defaults that never reach the symbol, edge values, saturated logits, properties (bit-reproducible,
loss-only, graph capture), ASPP_Classifier_V2.loss, the GALD decoder's heads, one ASPPTrainer / GALDTrainer step and one AsppFada iteration with
SOLVER.FOCAL_GAMMA set.

Bars: the family's (tests/test_gpu_wce.py) - loss and S 2e-5 relative, dlow 2e-5 of the expectation's largest magnitude.  torch's own fp32
evaluation of the formula lies at most 1.7e-7 (loss) / 3.3e-6 (dlow) from float64 on these shapes, the same at gamma 0: fp32 alone stays well inside."""
import functools
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _cases
import _focal_ref as R
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

LOSS_BAR, GRAD_BAR = 2e-5, 2e-5


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import kernels
    return kernels


def relmax(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


@functools.lru_cache(maxsize=None)
def inputs(name, confident=False):
    shape = R.SHAPE_BY_NAME[name]
    return R.confident_inputs(shape) if confident else R.shape_inputs(shape)


@functools.lru_cache(maxsize=None)
def shape_ref(name, gamma, weighted, confident=False):
    """(low, labels, weights or None, restatement, torch float64 (loss, dlow)) of one case: computed once, shared, never written to."""
    shape = R.SHAPE_BY_NAME[name]
    low, lab, w = inputs(name, confident)
    w = w if weighted else None
    return low, lab, w, R.focal_ref(low, lab, gamma, w, shape.align_corners), R.focal_torch(low, lab, gamma, w, shape.align_corners)


def fused(K, low, lab, gamma, w, align_corners, want_grad=True, **kw):
    """K.upsample_ce_focal on numpy operands -> (loss_out [4] numpy, dlow [B,h,w,K] numpy or None)."""
    out, dlow = K.upsample_ce_focal(torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), gamma, want_grad=want_grad, align_corners=align_corners,
                                    class_weights=None if w is None else torch.from_numpy(np.asarray(w, np.float32)).cuda(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if dlow is None else dlow.cpu().numpy()


def errors(r, out, dlow):
    loss, S = float(r.loss), float(r.S)
    e_loss = abs(float(out[0]) - loss) / abs(loss) if loss != 0.0 else abs(float(out[0]))
    e_S = abs(float(out[1]) - S) / S
    dmax = float(r.dlow.abs().max())
    e_d = relmax(dlow, r.dlow.numpy()) if dmax > 0 else float(np.abs(dlow).max())
    return e_loss, e_S, e_d


def check_against(r, out, dlow, what):
    assert np.isfinite(out[:3]).all() and np.isfinite(dlow).all(), what
    assert out[2] == float(r.bad), (what, out)
    e_loss, e_S, e_d = errors(r, out, dlow)
    print("%s: loss %.3e rel, S %.3e rel, dlow %.3e relmax" % (what, e_loss, e_S, e_d))
    assert e_loss < LOSS_BAR and e_S < LOSS_BAR and e_d < GRAD_BAR, (what, e_loss, e_S, e_d)


def check_against_torch(tloss, td, out, dlow, what):
    tl = float(tloss)
    e_loss = abs(float(out[0]) - tl) / abs(tl) if tl != 0.0 else abs(float(out[0]))
    e_d = relmax(dlow, td.numpy()) if float(td.abs().max()) > 0 else float(np.abs(dlow).max())
    print("%s vs torch float64: loss %.3e rel, dlow %.3e relmax" % (what, e_loss, e_d))
    assert e_loss < LOSS_BAR and e_d < GRAD_BAR, (what, e_loss, e_d)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "w"])
@pytest.mark.parametrize("gamma", R.GAMMAS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: s.name)
def test_parity_with_the_restatement_and_torch_float64(K, shape, gamma, weighted):
    low, lab, w, r, (tloss, td) = shape_ref(shape.name, gamma, weighted)
    out, dlow = fused(K, low, lab, gamma, w, shape.align_corners)
    what = "%s/gamma %g/%s" % (shape.name, gamma, "w" if weighted else "plain")
    check_against(r, out, dlow, what)
    if shape.K == 1:          # u is exactly 0: torch's pow has no gradient to give at 0 for gamma < 1; the loss is 0
        assert out[0] == 0.0 and not dlow.any()
    else:
        check_against_torch(tloss, td, out, dlow, what)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "w"])
@pytest.mark.parametrize("gamma", R.GAMMAS)
@pytest.mark.parametrize("name", R.CONFIDENT_SHAPES)
def test_parity_on_confident_pixels(K, name, gamma, weighted):
    """+8 on the label's own logit: u between about 1e-6 and 1e-1.  The reference here is the restatement, which forms u from the other classes
    as the kernel does; torch's composition (1 - exp(log q)) is printed beside it."""
    shape = R.SHAPE_BY_NAME[name]
    low, lab, w, r, (tloss, td) = shape_ref(name, gamma, weighted, True)
    out, dlow = fused(K, low, lab, gamma, w, shape.align_corners)
    what = "confident %s/gamma %g/%s" % (name, gamma, "w" if weighted else "plain")
    check_against(r, out, dlow, what)
    check_against_torch(tloss, td, out, dlow, what)


# ------------------------------------------------------------------------------------------------ 2. gamma = 0
def _raw(K, symbol, lowd, labd, cw, scalar, align_corners, want_grad=True):
    """mi_upsample_ce_focal / mi_upsample_ce_w themselves: `scalar` is gamma / label_smoothing."""
    from rnd_semantic_segmentation_amd import _lib
    B, h, w, Kc = lowd.shape
    _, H, W = labd.shape
    L = _lib.lib()
    ws = torch.empty(L.mi_upsample_ce_workspace(B, h, w, Kc, H, W), dtype=torch.uint8, device=lowd.device)
    out = torch.empty(4, dtype=torch.float32, device=lowd.device)
    dlow = torch.empty_like(lowd) if want_grad else None
    p = K._p
    _lib.check(getattr(L, symbol)(p(lowd), p(labd), p(cw), p(out), p(dlow), B, h, w, Kc, H, W, 255, float(scalar), 1.0, int(align_corners), p(ws),
                                  ws.numel(), K._stream()), symbol)
    torch.cuda.synchronize()
    return out, dlow


@pytest.mark.parametrize("name", ["k19_ac", "k19", "tiles_ac", "tiles", "k32"])
def test_gamma_zero_gives_the_bytes_of_the_weighted_and_the_plain_entry(K, name):
    shape = R.SHAPE_BY_NAME[name]
    low, lab, w = inputs(name)
    lowd, labd, wd = torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(w).cuda()
    want, want_d = _raw(K, "mi_upsample_ce_w", lowd, labd, wd, 0.0, shape.align_corners)
    got, got_d = _raw(K, "mi_upsample_ce_focal", lowd, labd, wd, 0.0, shape.align_corners)
    assert torch.equal(got[:3], want[:3]) and torch.equal(got_d, want_d)
    plain, plain_d = K.upsample_ce(lowd, labd, align_corners=shape.align_corners)          # mi_upsample_ce_ex
    torch.cuda.synchronize()
    got, got_d = _raw(K, "mi_upsample_ce_focal", lowd, labd, None, 0.0, shape.align_corners)
    assert torch.equal(got[:3], plain[:3]) and torch.equal(got_d, plain_d)
    lo, none = _raw(K, "mi_upsample_ce_focal", lowd, labd, None, 0.0, shape.align_corners, want_grad=False)
    assert none is None and torch.equal(lo[:3], plain[:3])
    # the wrapper at gamma 0 is the same call
    out, d = K.upsample_ce_focal(lowd, labd, 0.0, align_corners=shape.align_corners, class_weights=wd)
    torch.cuda.synchronize()
    assert torch.equal(out[:3], want[:3]) and torch.equal(d, want_d)


# ------------------------------------------------------------------------------------------------ 3. the defaults
def _tiny_aspp():
    from rnd_semantic_segmentation_amd.host import modules
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False, layers=(1, 1, 2, 2))
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], 19)
    for m in (fe, cls):
        synth.load_formula_weights(m)
        m.cuda()
        m.ensure_flat()
    return fe, cls


def _gald_inputs():
    x = torch.from_numpy(synth.synth_image(2, 224, 224, seed=5)).cuda()
    lab = torch.from_numpy(synth.synth_label(2, 224, 224, 19, seed=5)).long().cuda()
    return x, lab


def test_default_arguments_do_not_reach_the_new_symbol(K, monkeypatch):
    from rnd_semantic_segmentation_amd import _lib
    from rnd_semantic_segmentation_amd.host import gald
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab, w = inputs("k19_ac")
    lowd, labd, wd = torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(w).cuda()

    def refuse(*a):
        raise AssertionError("mi_upsample_ce_focal called")

    monkeypatch.setattr(_lib.lib(), "mi_upsample_ce_focal", refuse)
    out, dlow = K.upsample_ce(lowd, labd)
    K.upsample_ce(lowd, labd, class_weights=wd, label_smoothing=0.1)
    torch.cuda.synchronize()
    assert dlow is not None and np.isfinite(float(out[0]))
    with pytest.raises(AssertionError, match="mi_upsample_ce_focal called"):
        K.upsample_ce_focal(lowd, labd, 2.0)
    # ASPP_Classifier_V2.loss
    x, lab2 = _cases.net_inputs(2, 65, 11)
    labd2 = torch.from_numpy(lab2).cuda().long()
    fe, cls = _tiny_aspp()
    with torch.no_grad():
        feat = fe(torch.from_numpy(x).cuda()).detach()
    for kw in ({}, {"focal_gamma": 0.0}, {"class_weights": wd, "label_smoothing": 0.1}, {"ohem": (0.7, 100)}):
        assert np.isfinite(float(cls.loss(feat, labd2, 255, **kw).detach()))
    with pytest.raises(AssertionError, match="mi_upsample_ce_focal called"):
        cls.loss(feat, labd2, 255, focal_gamma=2.0)
    # GCPADecoder.losses / .loss
    xg, labg = _gald_inputs()
    torch.manual_seed(3)
    enc, dec = gald.GCPAEncoder().cuda().train(), gald.GCPADecoder().cuda().train()
    feats = enc(xg)
    for kw in ({}, {"focal_gamma": 0.0}, {"class_weights": wd}):
        assert all(np.isfinite(float(v.detach())) for v in dec.losses(xg, feats, labg, criterion="ce", **kw))
    assert np.isfinite(float(dec.loss(xg, feats, labg).detach()))
    with pytest.raises(AssertionError, match="mi_upsample_ce_focal called"):
        dec.losses(xg, feats, labg, criterion="ce", focal_gamma=2.0)
    with pytest.raises(AssertionError, match="mi_upsample_ce_focal called"):
        dec.loss(xg, feats, labg, focal_gamma=2.0)


# ------------------------------------------------------------------------------------------------ 4. edge values
def test_every_pixel_ignored_gives_nan_and_a_zero_gradient(K):
    low, lab, w = inputs("k19_ac")
    for weights in (None, w):
        out, dlow = fused(K, low, np.full_like(lab, 255), 2.0, weights, True)
        assert np.isnan(out[0]) and out[1] == 0.0 and out[2] == 0.0
        assert np.isfinite(dlow).all() and not dlow.any()
    # the identity scale, where a dlow row IS a pixel: the ignored pixel's row is exactly zero beside valid ones
    low2, lab2, w2 = inputs("ident")
    lab2 = np.full_like(lab2, int(np.flatnonzero(w2 > 0)[0]))
    lab2[0, 0, 1] = 255
    out2, dlow2 = fused(K, low2, lab2, 0.5, w2, False)
    assert np.isfinite(out2[0]) and not dlow2[0, 0, 1].any() and dlow2[0, 1, 0].any()
    check_against(R.focal_ref(low2, lab2, 0.5, w2, False), out2, dlow2, "identity with an ignored pixel")


def test_only_a_zero_weight_class_gives_nan(K):
    low, lab, w = inputs("k19_ac")
    zero = int(np.flatnonzero(w == 0)[0])
    out, dlow = fused(K, low, np.full_like(lab, zero), 2.0, w, True)
    assert np.isnan(out[0]) and out[1] == 0.0
    assert np.isfinite(dlow).all() and not dlow.any()
    assert np.isnan(float(R.focal_ref(low, np.full_like(lab, zero), 2.0, w, True).loss))


def test_out_of_range_labels_are_left_out_and_counted(K):
    low, lab, w = inputs("k19_ac")
    bad = lab.copy()
    bad.reshape(-1)[[3, 500, 501, 2000, 2969]] = [19, 254, -1, 1000, 2 ** 40]
    r = R.focal_ref(low, bad, 2.0, w, True)
    assert r.bad == 5
    out, dlow = fused(K, low, bad, 2.0, w, True)
    assert out[2] == 5.0
    check_against(r, out, dlow, "five bad labels")
    as_ignored = bad.copy()
    as_ignored[(bad < 0) | (bad >= 19)] = 255
    same, same_d = fused(K, low, as_ignored, 2.0, w, True)
    assert same[:2].tobytes() == out[:2].tobytes() and same_d.tobytes() == dlow.tobytes() and same[2] == 0.0


# ------------------------------------------------------------------------------------------------ 5. saturation
@pytest.mark.parametrize("gamma", [0.5, 5.0])
def test_logits_of_magnitude_80_stay_finite_and_within_five_times_torch_fp32(K, gamma):
    """Confidently wrong and confidently right pixels.  The allowance is five times the error torch's own fp32 evaluation of this case has
    against float64, computed here, with a floor of 2e-5: it belongs to the reference, not to the kernel."""
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab = R.make_inputs("focal.sat", shape.B, shape.K, shape.hw, shape.HW, magnitude=80.0)
    w = R.make_weights("focal.sat", shape.K)
    assert np.abs(low).max() == np.float32(80.0)
    r = R.focal_ref(low, lab, gamma, w, True)
    assert float(r.loss) > 10.0
    t32 = R.focal_torch(low, lab, gamma, w, True, dtype=torch.float32)
    t_loss = abs(float(t32[0]) - float(r.loss)) / float(r.loss)
    t_d = relmax(t32[1].numpy(), r.dlow.numpy())
    out, dlow = fused(K, low, lab, gamma, w, True)
    assert np.isfinite(out[:3]).all() and np.isfinite(dlow).all()
    e_loss, e_S, e_d = errors(r, out, dlow)
    print("magnitude 80, gamma %g: loss %.3e rel (torch fp32 %.3e), S %.3e rel, dlow %.3e relmax (torch fp32 %.3e)" % (gamma, e_loss, t_loss, e_S, e_d, t_d))
    assert e_loss <= max(5 * t_loss, 2e-5) and e_S < LOSS_BAR and e_d <= max(5 * t_d, 2e-5)


ZERO_U = R.SHAPES[0]._replace(name="zero_u", B=2, K=2, hw=(8, 9), HW=(8, 9), align_corners=True)          # identity: an entry's support is one pixel


@pytest.mark.parametrize("gamma", [0.5, 5.0])
def test_labels_at_the_argmax_of_magnitude_200_give_exact_zeros(K, gamma):
    """Every label is its pixel's argmax and the logits reach 200: where the other class's exponential underflows, u is exactly 0, and so are the
    pixel's loss term and gradient for every gamma (u^(gamma-1) is never formed).  An entry of dlow whose support holds only such pixels (or ignored
    ones) is exactly 0.  "Such" is decided in float64 with a margin: u < 1e-48, a gap above 110 (fp32 exponentials are 0 below a gap of 104).  With
    these inputs that is a quarter of the pixels, not most, and no entry of an upsampled shape sees only such pixels; at the identity scale with
    align_corners the source coordinate is the pixel's own in fp32 as in float64, every lambda is exactly 0 and an entry's support is its pixel.
    The same construction on k19_ac checks finiteness where supports overlap."""
    s = ZERO_U
    low, lab = R.make_inputs("focal.zero_u", s.B, s.K, s.hw, s.HW, magnitude=200.0)
    lab = np.where(lab == 255, lab, low.argmax(-1)).astype(np.int64)
    r = R.focal_ref(low, lab, gamma, None, True)
    dead = ((r.u < 1e-48) | torch.from_numpy(lab == 255)).numpy()
    frac = float((r.u.numpy()[lab != 255] < 1e-48).mean())
    print("u is exactly 0 on %.0f %% of the valid pixels; %d of %d dlow rows see only such pixels or ignored ones" % (100 * frac, dead.sum(), dead.size))
    assert frac > 0.1 and (~dead).sum() >= 10
    out, dlow = fused(K, low, lab, gamma, None, True)
    assert np.isfinite(out[:3]).all() and np.isfinite(dlow).all()
    assert not dlow[dead].any() and dlow[~dead].any()
    check_against(r, out, dlow, "magnitude 200 at the argmax, identity, gamma %g" % gamma)
    shape = R.SHAPE_BY_NAME["k19_ac"]
    low, lab = R.make_inputs("focal.zero_u19", shape.B, shape.K, shape.hw, shape.HW, magnitude=200.0)
    z = F.interpolate(torch.from_numpy(low).double().permute(0, 3, 1, 2), size=shape.HW, mode="bilinear", align_corners=True)
    lab = np.where(lab == 255, lab, z.argmax(1).numpy()).astype(np.int64)
    out, dlow = fused(K, low, lab, gamma, None, True)
    assert np.isfinite(out[:3]).all() and np.isfinite(dlow).all() and out[1] == float((lab != 255).sum())
    # printed, not judged: an interpolated logit of magnitude 200 is rounded to 1.5e-5 in fp32, u^gamma moves by gamma times that
    print("magnitude 200 at the argmax, k19_ac, gamma %g: loss %.3e rel, S %.3e rel, dlow %.3e relmax" % ((gamma,) + errors(R.focal_ref(low, lab, gamma, None, True), out, dlow)))


# ------------------------------------------------------------------------------------------------ 6. / 7. properties
def test_two_calls_are_bit_equal_and_loss_only_gives_the_same_bits(K):
    for name in ("k19", "tiles_ac", "f32"):
        shape = R.SHAPE_BY_NAME[name]
        low, lab, w = inputs(name)
        a, b = fused(K, low, lab, 2.0, w, shape.align_corners), fused(K, low, lab, 2.0, w, shape.align_corners)
        assert a[0][:3].tobytes() == b[0][:3].tobytes() and a[1].tobytes() == b[1].tobytes()
        out, dlow = fused(K, low, lab, 2.0, w, shape.align_corners, want_grad=False)
        assert dlow is None and out[:3].tobytes() == a[0][:3].tobytes()


def test_the_call_is_capturable_and_a_replay_reads_its_operands_anew(K):
    shape = R.SHAPE_BY_NAME["k19"]
    low, lab, w, r, _ = shape_ref("k19", 2.0, True)
    other_low, other_lab = R.make_inputs("focal.graph", shape.B, shape.K, shape.hw, shape.HW)
    lowd, labd = torch.from_numpy(other_low).cuda(), torch.from_numpy(other_lab).cuda()
    wd = torch.ones(shape.K, device="cuda")
    K.upsample_ce_focal(lowd, labd, 2.0, align_corners=False, class_weights=wd)          # outside the capture: code objects, LDS attribute
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, dlow = K.upsample_ce_focal(lowd, labd, 2.0, align_corners=False, class_weights=wd)
    graph.replay()
    torch.cuda.synchronize()
    first_out, first_d = K.upsample_ce_focal(lowd.clone(), labd.clone(), 2.0, align_corners=False, class_weights=torch.ones(shape.K, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(out[:3], first_out[:3]) and torch.equal(dlow, first_d)
    lowd.copy_(torch.from_numpy(low))          # in place: the captured pointers, new values
    labd.copy_(torch.from_numpy(lab))
    wd.copy_(torch.from_numpy(w))
    graph.replay()
    torch.cuda.synchronize()
    eager_out, eager_d = K.upsample_ce_focal(torch.from_numpy(low).cuda(), torch.from_numpy(lab).cuda(), 2.0, align_corners=False,
                                             class_weights=torch.from_numpy(w).cuda())
    torch.cuda.synchronize()
    assert torch.equal(out[:3], eager_out[:3]) and torch.equal(dlow, eager_d) and not torch.equal(out[:2], first_out[:2])
    check_against(r, out.cpu().numpy(), dlow.cpu().numpy(), "graph replay with new logits, labels and weights")


# ------------------------------------------------------------------------------------------------ 8. layers
def _nhwc(low_nchw):
    return low_nchw.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()


def test_aspp_classifier_loss_with_focal_weights_and_temperature(K):
    """ASPP_Classifier_V2.loss(focal_gamma=2, temperature=1.8, class_weights=w) against the restatement on its own last_low / 1.8 (the division comes
    first), and the gradient that reaches the head's bias against the restatement's dlow / 1.8 summed over B, h, w."""
    T = 1.8
    x, lab = _cases.net_inputs(2, 129, 71)
    labd = torch.from_numpy(lab).cuda().long()
    w = R.make_weights("focal.aspp", 19)
    fe, cls = _tiny_aspp()
    with torch.no_grad():
        feat = fe(torch.from_numpy(x).cuda()).detach()
    loss = cls.loss(feat, labd, 255, focal_gamma=2, temperature=T, class_weights=torch.from_numpy(w).cuda())
    loss.backward()
    torch.cuda.synchronize()
    plain = _tiny_aspp()[1].loss(feat, labd, 255, temperature=T, class_weights=torch.from_numpy(w).cuda())
    low = _nhwc(cls.last_low)
    assert low.shape == (2, 17, 17, 19)
    r = R.focal_ref(low.astype(np.float64) / T, lab, 2.0, w, True)
    e_loss = abs(float(loss) - float(r.loss)) / float(r.loss)
    print("ASPP head: loss %.6f (gamma 0: %.6f), %.3e rel" % (float(loss), float(plain), e_loss))
    assert e_loss < LOSS_BAR and float(loss) < float(plain)
    # each branch bias receives the sum of d loss / d low over B, h, w (an fp32 column sum, as tests/test_gpu_wce.py relies on)
    got_b = dict(cls.named_parameters())["conv2d_list.0.bias"].grad.detach().cpu().numpy()
    want_b = r.dlow.sum((0, 1, 2)).numpy() / T
    e_b = relmax(got_b, want_b)
    print("ASPP head: bias gradient %.3e relmax" % e_b)
    assert e_b < GRAD_BAR


def test_decoder_heads_with_focal_match_the_restatement_on_their_own_logits(K):
    """GCPAEncoder + GCPADecoder, 2 x 3 x 224 x 224, criterion="ce" with focal_gamma=2: each of the four losses equals the restatement on the tapped
    low-resolution logits (linear5 .. linear2), and after backward each head's bias gradient equals the restatement's dlow summed over B, h, w and
    weighted 0.4 / 0.6 / 0.8 / 1 (fp32 on the tape, as in test_gpu_wce.py)."""
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()
    torch.manual_seed(3)
    enc, dec = gald.GCPAEncoder().cuda().train(), gald.GCPADecoder().cuda().train()
    with torch.no_grad():
        dec.long_relation.gamma.fill_(0.3)
    dec._taps = {}
    ls = dec.losses(x, enc(x), lab, criterion="ce", focal_gamma=2)
    (ls[3] * 1 + ls[2] * 0.8 + ls[1] * 0.6 + ls[0] * 0.4).backward()
    torch.cuda.synchronize()
    assert dec.__dict__.get("bad_labels") is not None and float(dec.bad_labels) == 0.0
    labn = lab.cpu().numpy()
    for loss, i, weight in zip(ls, (5, 4, 3, 2), (0.4, 0.6, 0.8, 1.0)):
        low = dec._taps["linear%d" % i].t.detach().cpu().numpy()
        r = R.focal_ref(low, labn, 2.0, None, False)
        e_loss = abs(float(loss) - float(r.loss)) / float(r.loss)
        want = r.dlow.sum((0, 1, 2)).numpy() * weight
        e_b = relmax(getattr(dec, "linear%d" % i).bias.grad.cpu().numpy(), want)
        print("linear%d: loss %.6f, %.3e rel; bias gradient %.3e relmax" % (i, float(loss), e_loss, e_b))
        assert e_loss < LOSS_BAR and e_b < GRAD_BAR, (i, e_loss, e_b)


# ------------------------------------------------------------------------------------------------ 9. trainers
def _cfg(tmp_path, *opts, yaml=None):
    from rnd_semantic_segmentation_amd.host import config as hc
    cfg = hc.CfgNode(hc.default_tree())
    if yaml:
        cfg.merge_from_file(yaml)
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "MODEL.NUM_CLASSES", 19, "MODEL.FREEZE_BN", True, "SOLVER.EPOCHS", 1, "SOLVER.BASE_LR", 1e-4] + list(opts))
    cfg.freeze()
    return cfg


WEIGHTS = R.make_weights("focal.trainer", 19)
FOCAL = ["SOLVER.FOCAL_GAMMA", 2.0, "SOLVER.CLASS_WEIGHTS", str(tuple(float(v) for v in WEIGHTS))]


def test_aspp_trainer_step_with_the_key_set_and_at_its_default(K, tmp_path):
    from rnd_semantic_segmentation_amd.host import modules
    from rnd_semantic_segmentation_amd.host.trainer import ASPPTrainer

    class Tiny(ASPPTrainer):
        build_feature_extractor = staticmethod(lambda cfg: modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False,
                                                                                            layers=(1, 1, 2, 2)))

    x, lab = _cases.net_inputs(2, 65, 11)
    xt, lt = torch.from_numpy(x), torch.from_numpy(lab)

    def make(*opts):
        tr = Tiny("aspp", _cfg(tmp_path, *opts), [None] * 50, 0, logger=logging.getLogger("focal-aspp"))
        with torch.no_grad():
            for m in (tr.feature_extractor, tr.classifier):
                synth.load_formula_weights(m)
                m._store.generation += 1
        return tr

    tr = make(*FOCAL)
    assert tr.focal_gamma == 2.0 and set(tr.ce_kwargs) == {"focal_gamma", "class_weights"} and tr.ce_weights.is_cuda
    before = tr.classifier._store.data.clone()
    loss, _ = tr.train_step(xt, lt, 40)
    torch.cuda.synchronize()
    r = R.focal_ref(_nhwc(tr.classifier.last_low), lab, 2.0, WEIGHTS, True)
    e_loss = abs(float(loss) - float(r.loss)) / float(r.loss)
    print("ASPPTrainer: loss %.6f, %.3e rel to the restatement on the captured logits" % (float(loss), e_loss))
    assert e_loss < LOSS_BAR and not torch.equal(before, tr.classifier._store.data)
    never, zero = make(), make("SOLVER.FOCAL_GAMMA", 0.0)
    assert never.ce_kwargs == {} and zero.ce_kwargs == {}
    loss0, _ = never.train_step(xt, lt, 40)
    loss00, _ = zero.train_step(xt, lt, 40)
    torch.cuda.synchronize()
    assert torch.equal(loss0, loss00) and float(loss0) != float(loss)
    assert torch.equal(never.classifier._store.data, zero.classifier._store.data)


def test_gald_trainer_step_with_the_key_set_and_at_its_default(K, tmp_path):
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()

    def make(*opts):
        log = logging.getLogger("focal-gald")
        log.addHandler(logging.NullHandler())
        torch.manual_seed(11)
        tr = gald.GALDTrainer("gald", _cfg(tmp_path, *opts), None, 0, logger=log)
        tr.encoder.train()
        tr.decoder.train()
        return tr

    tr = make("SOLVER.FOCAL_GAMMA", 2.0)
    assert tr.ce_kwargs == {"focal_gamma": 2.0}
    before = tr.decoder._store.data.clone()
    tr.decoder._taps = {}
    loss, _ = tr.train_step(x, lab, 100)
    torch.cuda.synchronize()
    assert gald.take_bad_labels(tr.decoder, tr.criterion) == 0
    labn, want = lab.cpu().numpy(), 0.0
    for i, weight in zip((5, 4, 3, 2), (0.4, 0.6, 0.8, 1.0)):
        want += weight * float(R.focal_ref(tr.decoder._taps["linear%d" % i].t.detach().cpu().numpy(), labn, 2.0, None, False).loss)
    e_loss = abs(float(loss) - want) / want
    print("GALDTrainer: loss %.6f, %.3e rel to the restatement on the captured logits" % (float(loss), e_loss))
    assert e_loss < LOSS_BAR and not torch.equal(before, tr.decoder._store.data)
    never, zero = make(), make("SOLVER.FOCAL_GAMMA", 0.0)
    loss0, _ = never.train_step(x, lab, 100)
    loss00, _ = zero.train_step(x, lab, 100)
    torch.cuda.synchronize()
    assert torch.equal(loss0, loss00) and float(loss0) != float(loss)


# ------------------------------------------------------------------------------------------------ 10. FADA
def _combo(tmp_path, monkeypatch, *opts):
    """AsppFada on the product modules (tiny depth plan, formula weights), as tests/test_gpu_fada.py configures it."""
    from rnd_semantic_segmentation_amd.host import config as hc
    from rnd_semantic_segmentation_amd.host import fada, modules
    from rnd_semantic_segmentation_amd.host import trainer as tr
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "deeplabv2_r101_adv.yaml"))
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "SOLVER.BASE_LR", 5e-4, "SOLVER.BASE_LR_D", 1e-4] + list(opts))
    cfg.freeze()

    def formula(m):
        synth.load_formula_weights(m)
        return m

    monkeypatch.setattr(tr.ASPPTrainer, "build_feature_extractor", staticmethod(
        lambda cfg: formula(modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False, layers=(1, 1, 1, 1)))))
    monkeypatch.setattr(tr.ASPPTrainer, "build_classifier", staticmethod(lambda cfg: formula(modules.build_classifier(cfg))))
    monkeypatch.setattr(fada.FADAAdapter, "build_adversarial_discriminator", staticmethod(lambda cfg: formula(fada.build_adversarial_discriminator(cfg))))
    monkeypatch.setattr(fada, "setup_logger", lambda *a, **k: logging.getLogger("test_gpu_focal"))
    return fada.AsppFada("aspp_fada", cfg, [], [], 0)


def test_one_fada_iteration_with_the_key_set(K, tmp_path, monkeypatch):
    """loss_seg is the focal loss of the source logits / T (the restatement on the classifier's last_low, captured before the target pass overwrites
    it); the adversarial and discriminator losses of the first iteration depend on the forward passes alone and keep their bits."""
    xs, ys = synth.synth_image(2, 65, 65, seed=51), synth.synth_label(2, 65, 65, 19, seed=51)
    xt = torch.from_numpy(synth.synth_image(2, 65, 65, seed=52))
    plain = _combo(tmp_path, monkeypatch).train_step(torch.from_numpy(xs), torch.from_numpy(ys), xt, 40)
    combo = _combo(tmp_path, monkeypatch, *FOCAL)
    assert combo.aspp.focal_gamma == 2.0 and set(combo.aspp.ce_kwargs) == {"focal_gamma", "class_weights"}
    cls, captured = combo.aspp.classifier, []
    real_loss = cls.loss

    def tap(*a, **kw):
        out = real_loss(*a, **kw)
        captured.append((_nhwc(cls.last_low), kw))
        return out

    monkeypatch.setattr(cls, "loss", tap)
    got = combo.train_step(torch.from_numpy(xs), torch.from_numpy(ys), xt, 40)
    torch.cuda.synchronize()
    assert len(captured) == 1 and captured[0][1]["focal_gamma"] == 2.0 and captured[0][1]["temperature"] == combo.TEMPERATURE
    low = captured[0][0]
    ns = xs.shape[0]
    r = R.focal_ref(low[:ns].astype(np.float64) / combo.TEMPERATURE, ys.astype(np.int64), 2.0, WEIGHTS, True)
    e_loss = abs(float(got["loss_seg"]) - float(r.loss)) / float(r.loss)
    print("AsppFada: loss_seg %.6f (cross-entropy %.6f), %.3e rel to the restatement" % (float(got["loss_seg"]), float(plain["loss_seg"]), e_loss))
    assert e_loss < LOSS_BAR and float(got["loss_seg"]) != float(plain["loss_seg"])
    for k in ("loss_adv_tgt", "loss_D_src", "loss_D_tgt"):
        a, b = torch.as_tensor(got[k]).detach().cpu(), torch.as_tensor(plain[k]).detach().cpu()
        assert torch.equal(a, b), (k, float(a), float(b))
