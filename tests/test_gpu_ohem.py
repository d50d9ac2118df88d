"""GPU tests of online hard example mining in the fused upsample + cross-entropy heads (mi_upsample_ce_ohem, csrc/upsample_ce.hip) and the layers
above it: K.upsample_ce_ohem against the float64 restatement (tests/_ohem_ref.py) and F.cross_entropy on the kept pixels in float64, the selection
checked exactly on the kernel's own probabilities, the everything-kept call against K.upsample_ce, edge values, properties (bit-reproducible,
loss-only, graph capture with `low` read at replay), ASPP_Classifier_V2.loss(ohem=), the GALD decoder's heads, and one ASPPTrainer / GALDTrainer step
with SOLVER.LOSS ohem.

Bars: those of tests/test_gpu_wce.py / test_gpu_gdl.py - loss and t 2e-5 relative, dlow 2e-5 of the expectation's largest magnitude; n_kept and the
bad-label count equal.  Every parity case keeps a relative 1e-4 between t and the nearest other q (tests/test_host_ohem.py::test_margin_condition),
so float64 and the kernel keep the same pixels."""
import functools
import logging

import numpy as np
import pytest
import torch

import _cases
import _ohem_ref as R
from _wce_ref import SHAPE_BY_NAME, make_inputs
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

LOSS_BAR = GRAD_BAR = R.PARITY_BAR
NAMES = [c.name for c in R.CASES]


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
def autograd_ref(name):
    low, lab, _, _ = R.case_inputs(name)
    return R.ohem_autograd(low, lab, R.case_ref(name).kept, R.CASE_BY_NAME[name].shape.align_corners)


def fused(K, low, lab, thresh, min_kept, align_corners, want_grad=True, want_prob=False, **kw):
    """K.upsample_ce_ohem on numpy operands -> (loss_out [4], dlow [B,h,w,K] or None, prob [B,H,W] or None) as numpy."""
    out, dlow, prob = K.upsample_ce_ohem(torch.from_numpy(np.array(low)).cuda(), torch.from_numpy(np.array(lab)).cuda(), thresh, min_kept,
                                         want_grad=want_grad, align_corners=align_corners, want_prob=want_prob, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if dlow is None else dlow.cpu().numpy(), None if prob is None else prob.cpu().numpy()


def check_against(r, out, dlow, what):
    assert np.isfinite(out).all() and np.isfinite(dlow).all(), what
    loss, t = float(r.loss), float(r.t)
    e_loss = abs(float(out[0]) - loss) / abs(loss) if loss != 0.0 else abs(float(out[0]))
    e_t = abs(float(out[3]) - t) / t if t != 0.0 else abs(float(out[3]))
    dmax = float(r.dlow.abs().max())
    e_d = relmax(dlow, r.dlow.numpy()) if dmax > 0 else float(np.abs(dlow).max())
    print("%s: loss %.3e rel, t %.3e rel, dlow %.3e relmax, n_kept %d (want %d), bad %d (want %d)" % (what, e_loss, e_t, e_d, out[1], r.n_kept, out[2], r.bad))
    assert out[1] == float(r.n_kept) and out[2] == float(r.bad), (what, out, r.n_kept, r.bad)
    assert e_loss < LOSS_BAR and e_t < LOSS_BAR and e_d < GRAD_BAR, (what, e_loss, e_t, e_d)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", NAMES)
def test_parity_with_the_restatement_and_torch_float64(K, name):
    low, lab, thresh, min_kept = R.case_inputs(name)
    ac = R.CASE_BY_NAME[name].shape.align_corners
    r = R.case_ref(name)
    out, dlow, _ = fused(K, low, lab, thresh, min_kept, ac)
    check_against(r, out, dlow, name)
    tloss, td = autograd_ref(name)
    tl = float(tloss)
    e_loss = abs(float(out[0]) - tl) / abs(tl) if tl != 0.0 else abs(float(out[0]))
    e_d = relmax(dlow, td.numpy()) if float(td.abs().max()) > 0 else float(np.abs(dlow).max())
    print("%s vs F.cross_entropy on the kept pixels, float64: loss %.3e rel, dlow %.3e relmax" % (name, e_loss, e_d))
    assert e_loss < LOSS_BAR and e_d < GRAD_BAR, (e_loss, e_d)


# ------------------------------------------------------------------------------------------------ 2. the selection, exactly
def _valid(lab, K_):
    return (lab != 255) & (lab >= 0) & (lab < K_)


def _check_selection(out, prob, lab, K_, thresh, min_kept, what):
    """t and n_kept from the kernel's own q, on the host, with no float64 in between."""
    valid = _valid(lab, K_)
    assert prob.dtype == np.float32 and (prob[~valid] == np.float32(2.0)).all() and (prob[valid] <= 1.0).all() and (prob[valid] >= 0.0).all()
    qs = np.sort(prob[valid])
    k = min(min_kept, qs.size)
    t = max(np.float32(thresh), qs[k - 1]) if k else np.float32(thresh)
    n_kept = int((prob[valid] <= t).sum())
    print("%s: k %d of %d valid, t %.9g (kernel %.9g), n_kept %d (kernel %d)" % (what, k, qs.size, t, out[3], n_kept, out[1]))
    assert np.float32(out[3]).tobytes() == np.float32(t).tobytes(), (what, out[3], t)
    assert out[1] == float(n_kept) and n_kept >= k
    return valid & (prob <= t)


SELECTION = [("k19-minkept", None), ("k19_ac-thresh", None), ("k19-all", None), ("tiles-minkept", None), ("f32-minkept", None), ("k32-minkept", None),
             ("cluster", None), ("cluster", 3), ("cluster", 1000), ("ties", None), ("ties", 1), ("many_wg", None), ("second_trip", None), ("second_trip", 3)]


@pytest.mark.parametrize("name,divisor", SELECTION, ids=["%s%s" % (n, "" if d is None else "-n/%d" % d) for n, d in SELECTION])
def test_threshold_and_count_are_exact_on_the_kernels_own_probabilities(K, name, divisor):
    """divisor: min_kept = n // divisor instead of the case's own (thresh 0), so that the order statistic decides - in the cluster and ties cases too,
    where no float64 comparison can."""
    low, lab, thresh, min_kept = R.case_inputs(name)
    shape = R.CASE_BY_NAME[name].shape
    if divisor is not None:
        thresh, min_kept = 0.0, max(1, int(_valid(lab, shape.K).sum()) // divisor)
    out, _, prob = fused(K, low, lab, thresh, min_kept, shape.align_corners, want_prob=True)
    _check_selection(out, prob, lab, shape.K, thresh, min_kept, name)
    r = R.case_ref(name)
    v = _valid(lab, shape.K)
    assert np.abs(prob[v] - r.q.numpy()[v]).max() < LOSS_BAR          # the stored q is the restatement's


@pytest.mark.parametrize("setting", ["minkept", "thresh", "cluster", "ties"])
def test_only_kept_pixels_receive_gradient(K, setting):
    """Identity geometry (h == H, w == W): a row of dlow is a pixel.  The rows that are not zero are kept pixels, and there are n_kept of them."""
    B, Kc, HW = 2, 19, (33, 45)
    low, lab = make_inputs("ohem.identity", B, Kc, HW, HW, magnitude=1e-3 if setting == "cluster" else None)
    if setting == "ties":
        low = np.full_like(low, -0.5)
    n = int(_valid(lab, Kc).sum())
    thresh, min_kept = {"minkept": (0.0, n // 3), "thresh": (0.1, 1), "cluster": (0.0, n // 3), "ties": (0.0, 5)}[setting]
    out, dlow, prob = fused(K, low, lab, thresh, min_kept, False, want_prob=True)
    kept = _check_selection(out, prob, lab, Kc, thresh, min_kept, "identity/" + setting)
    touched = dlow.any(-1)
    assert not (touched & ~kept).any()
    assert int(touched.sum()) == int(kept.sum()) == int(out[1])          # softmax - onehot is nowhere all zero at these magnitudes
    assert (dlow[~kept] == 0.0).all()
    if setting == "ties":
        assert int(out[1]) == n


# ------------------------------------------------------------------------------------------------ 3. everything kept: the plain cross-entropy
@pytest.mark.parametrize("name", ["k19_ac", "k19", "k32", "tiles_ac", "tiles", "f32"])
def test_everything_kept_is_the_plain_fused_cross_entropy(K, name):
    low, lab, thresh, min_kept = R.case_inputs(name + "-all")
    shape = SHAPE_BY_NAME[name]
    out, dlow, _ = fused(K, low, lab, thresh, min_kept, shape.align_corners)
    want, want_d = K.upsample_ce(torch.from_numpy(np.array(low)).cuda(), torch.from_numpy(np.array(lab)).cuda(), align_corners=shape.align_corners)
    torch.cuda.synchronize()
    want, want_d = want.cpu().numpy(), want_d.cpu().numpy()
    e_loss, e_d = abs(float(out[0]) - float(want[0])) / float(want[0]), relmax(dlow, want_d)
    print("%s: against K.upsample_ce: loss %.3e rel, dlow %.3e relmax, n_kept %d, n_valid %d" % (name, e_loss, e_d, out[1], want[1]))
    assert out[1] == want[1] and out[2] == want[2] == 0.0
    assert e_loss < LOSS_BAR and e_d < GRAD_BAR


# ------------------------------------------------------------------------------------------------ 4. edge values
def test_every_pixel_ignored_gives_nan_and_a_zero_gradient(K):
    low, lab, _, _ = R.case_inputs("k19_ac-all")
    out, dlow, prob = fused(K, low, np.full_like(lab, 255), 0.3, 10, True, want_prob=True)
    assert np.isnan(out[0]) and out[1] == 0.0 and out[2] == 0.0 and out[3] == np.float32(0.3)
    assert np.isfinite(dlow).all() and not dlow.any() and (prob == 2.0).all()


def test_out_of_range_labels_are_left_out_and_counted(K):
    low, lab, _, _ = R.case_inputs("k19_ac-all")
    bad = lab.copy()
    bad.reshape(-1)[[3, 500, 501, 2000, 2969]] = [19, 254, -1, 1000, 2 ** 40]
    r = R.ohem_ref(low, bad, 0.0, 40, True)
    assert r.bad == 5 and r.n_kept == 40 and r.margin >= R.MARGIN
    out, dlow, prob = fused(K, low, bad, 0.0, 40, True, want_prob=True)
    assert out[2] == 5.0 and (prob.reshape(-1)[[3, 500, 501, 2000, 2969]] == 2.0).all()
    check_against(r, out, dlow, "five bad labels")
    as_ignored = bad.copy()
    as_ignored[(bad < 0) | (bad >= 19)] = 255
    same, same_d, _ = fused(K, low, as_ignored, 0.0, 40, True)
    assert same[[0, 1, 3]].tobytes() == out[[0, 1, 3]].tobytes() and same_d.tobytes() == dlow.tobytes() and same[2] == 0.0
    from rnd_semantic_segmentation_amd import kernels
    with pytest.raises(ValueError, match="5 label values"):
        kernels.check_labels(torch.from_numpy(out), 19)


def test_logits_of_magnitude_80_stay_finite(K):
    """A confidently wrong pixel: q underflows to 0 in fp32, its loss term is formed as log(sum exp) - (z_y - max) and stays finite.  Everything kept
    (so that float64 and fp32 cannot disagree about a pixel beside t), and the mining settings for finiteness."""
    shape = SHAPE_BY_NAME["k19_ac"]
    low, lab = make_inputs("ohem.sat", shape.B, shape.K, shape.hw, shape.HW, magnitude=80.0)
    assert np.abs(low).max() == np.float32(80.0)
    n = int((lab != 255).sum())
    r = R.ohem_ref(low, lab, 0.0, 10 * n, True)
    assert float(r.loss) > 10.0 and r.n_kept == n
    out, dlow, prob = fused(K, low, lab, 0.0, 10 * n, True, want_prob=True)
    assert (prob == 0.0).any()
    check_against(r, out, dlow, "magnitude 80")
    for thresh, min_kept in ((0.7, 1), (0.0, n // 3)):
        out, dlow, prob = fused(K, low, lab, thresh, min_kept, True, want_prob=True)
        assert np.isfinite(out).all() and np.isfinite(dlow).all() and out[0] > 10.0
        _check_selection(out, prob, lab, shape.K, thresh, min_kept, "magnitude 80 (%g, %d)" % (thresh, min_kept))


def test_min_kept_one_with_thresh_zero_keeps_the_pixels_tied_for_the_minimum(K):
    low, lab, _, _ = R.case_inputs("k19-all")
    tied = []
    for lo, la in ((low, lab), (low[:1], lab[:1])):
        out, _, prob = fused(K, lo, la, 0.0, 1, False, want_prob=True)
        v = _valid(la, 19)
        tied.append(int((prob[v] == prob[v].min()).sum()))          # (a clamped border of the align_corners=False geometry repeats a pixel: more than one may tie)
        assert out[3] == prob[v].min() and out[1] == float(tied[-1]) and 1 <= tied[-1] < 10
    # twice as many pixels share the smallest q: the first image and a copy of it
    low2, lab2 = np.concatenate([low[:1], low[:1]]), np.concatenate([lab[:1], lab[:1]])
    out, dlow, prob = fused(K, low2, lab2, 0.0, 1, False, want_prob=True)
    v = _valid(lab2, 19)
    assert out[3] == prob[v].min() and out[1] == 2.0 * tied[1] and (prob[0] == prob[1]).all() and dlow[0].tobytes() == dlow[1].tobytes()
    lowt, labt, _, _ = R.case_inputs("ties")
    out, _, prob = fused(K, lowt, labt, 0.0, 1, False, want_prob=True)
    assert out[1] == float(_valid(labt, 19).sum()) and out[3] == prob[_valid(labt, 19)][0]


# ------------------------------------------------------------------------------------------------ 5. properties
def test_two_calls_are_bit_equal_and_loss_only_gives_the_same_bits(K):
    for name in ("k19-minkept", "tiles_ac-minkept", "f32-minkept", "many_wg", "second_trip", "cluster"):
        low, lab, thresh, min_kept = R.case_inputs(name)
        ac = R.CASE_BY_NAME[name].shape.align_corners
        a, b = fused(K, low, lab, thresh, min_kept, ac, want_prob=True), fused(K, low, lab, thresh, min_kept, ac, want_prob=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name
        out, dlow, prob = fused(K, low, lab, thresh, min_kept, ac, want_grad=False)
        assert dlow is None and prob is None and out.tobytes() == a[0].tobytes(), name


def test_the_call_is_capturable_and_a_replay_reads_low_anew(K):
    low, lab, thresh, min_kept = R.case_inputs("many_wg")
    low2, _ = make_inputs("ohem.replay", *[getattr(R.MANY_WG, f) for f in ("B", "K", "hw", "HW")])
    lowd, labd = torch.from_numpy(np.array(low)).cuda(), torch.from_numpy(np.array(lab)).cuda()
    K.upsample_ce_ohem(lowd, labd, thresh, min_kept, align_corners=False, want_prob=True)          # outside the capture: code objects, LDS attribute
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, dlow, prob = K.upsample_ce_ohem(lowd, labd, thresh, min_kept, align_corners=False, want_prob=True)
    graph.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in (out, dlow, prob)]
    eager = K.upsample_ce_ohem(torch.from_numpy(np.array(low)).cuda(), labd, thresh, min_kept, align_corners=False, want_prob=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, eager))
    check_against(R.case_ref("many_wg"), out.cpu().numpy(), dlow.cpu().numpy(), "graph replay")
    lowd.copy_(torch.from_numpy(low2))          # in place: the captured pointer, new values
    graph.replay()
    torch.cuda.synchronize()
    eager2 = K.upsample_ce_ohem(torch.from_numpy(low2).cuda(), labd, thresh, min_kept, align_corners=False, want_prob=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((out, dlow, prob), eager2)) and not torch.equal(out[:1], first[0][:1])


def test_default_arguments_do_not_reach_the_new_symbol(K, monkeypatch):
    from rnd_semantic_segmentation_amd import _lib
    low, lab, _, _ = R.case_inputs("k19_ac-all")
    lowd, labd = torch.from_numpy(np.array(low)).cuda(), torch.from_numpy(np.array(lab)).cuda()

    def refuse(*a):
        raise AssertionError("mi_upsample_ce_ohem called")

    monkeypatch.setattr(_lib.lib(), "mi_upsample_ce_ohem", refuse)
    out, dlow = K.upsample_ce(lowd, labd)
    out2, _ = K.upsample_ce(lowd, labd, class_weights=None, label_smoothing=0.0, want_grad=False)
    K.upsample_ce(lowd, labd, label_smoothing=0.1)
    K.upsample_gdl(lowd, labd)
    torch.cuda.synchronize()
    assert torch.equal(out[:3], out2[:3]) and dlow is not None
    with pytest.raises(AssertionError, match="mi_upsample_ce_ohem called"):
        K.upsample_ce_ohem(lowd, labd, 0.7, 100)


# ------------------------------------------------------------------------------------------------ 6. layers
def _tiny_aspp():
    from rnd_semantic_segmentation_amd.host import modules
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False, layers=(1, 1, 2, 2))
    cls = modules.ASPP_Classifier_V2(2048, [6, 12, 18, 24], [6, 12, 18, 24], 19)
    for m in (fe, cls):
        synth.load_formula_weights(m)
        m.cuda()
        m.ensure_flat()
    return fe, cls


def test_aspp_classifier_loss_with_ohem_and_temperature(K):
    """ASPP_Classifier_V2.loss(ohem=) (C = 2048 head on the 17 x 17 feature of the tiny backbone at 129 x 129) at temperature 1.8 against the
    restatement on the head's own low-resolution logits divided by 1.8: loss, n_kept, t, and the gradient that reaches the head's bias
    (the sum of d loss / d low over B, h, w, times 1 / T).  min_kept decides (a quarter of the valid pixels), so n_kept is min_kept on both sides."""
    T = 1.8
    x, lab = _cases.net_inputs(2, 129, 71)
    labd = torch.from_numpy(lab).cuda().long()
    n = int((lab != 255).sum())
    ohem = (0.0, n // 4)
    fe, cls = _tiny_aspp()
    with torch.no_grad():
        feat = fe(torch.from_numpy(x).cuda()).detach()
    loss = cls.loss(feat, labd, 255, temperature=T, ohem=ohem)
    loss.backward()
    torch.cuda.synchronize()
    got_b = dict(cls.named_parameters())["conv2d_list.0.bias"].grad.detach().cpu().numpy()
    out = cls._engine.last_loss_out.cpu().numpy()
    low = cls.last_low.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    r = R.ohem_ref(low / T, lab, ohem[0], ohem[1], True)
    plain = _tiny_aspp()[1].loss(feat, labd, 255, temperature=T)
    loss = loss.detach()
    e_loss, e_t = abs(float(loss) - float(r.loss)) / float(r.loss), abs(float(out[3]) - r.t) / r.t
    e_b = relmax(got_b, r.dlow.sum((0, 1, 2)).numpy() / T)
    print("ASPP head: ohem loss %.6f (plain %.6f), %.3e rel; t %.6g, %.3e rel; n_kept %d (want %d); margin %.3e; bias gradient %.3e relmax"
          % (float(loss), float(plain), e_loss, r.t, e_t, out[1], r.n_kept, r.margin, e_b))
    assert out[1] == float(r.n_kept) and ohem[1] <= r.n_kept < ohem[1] + 8 and out[2] == 0.0          # (min_kept, and what ties with the last of them)
    assert e_loss < LOSS_BAR and e_t < LOSS_BAR and e_b < GRAD_BAR, (e_loss, e_t, e_b)
    assert float(loss) > float(plain)          # the mean over the hardest quarter


def _gald_inputs():
    x = torch.from_numpy(synth.synth_image(2, 224, 224, seed=5)).cuda()
    lab = torch.from_numpy(synth.synth_label(2, 224, 224, 19, seed=5)).long().cuda()
    return x, lab


def test_decoder_heads_with_ohem_match_the_restatement_on_their_own_logits(K):
    """GCPAEncoder + GCPADecoder, 2 x 3 x 224 x 224, criterion="ohem": each of the four losses equals the restatement on the tapped low-resolution
    logits (linear5 .. linear2), each head mining on its own; after backward each head's bias gradient equals the restatement's dlow summed over
    B, h, w and weighted 0.4 / 0.6 / 0.8 / 1.  Then loss(), the single-head form, with a temperature."""
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()
    labn = lab.cpu().numpy()
    n = int((labn != 255).sum())
    ohem = (0.0, n // 4)
    torch.manual_seed(3)
    enc, dec = gald.GCPAEncoder().cuda().train(), gald.GCPADecoder().cuda().train()
    with torch.no_grad():
        dec.long_relation.gamma.fill_(0.3)
    dec._taps = {}
    feats = enc(x)
    plain = [float(v) for v in dec.losses(x, feats, lab, criterion="ce")]
    dec._taps = {}
    ls = dec.losses(x, feats, lab, criterion="ohem", ohem=ohem)
    (ls[3] * 1 + ls[2] * 0.8 + ls[1] * 0.6 + ls[0] * 0.4).backward()
    torch.cuda.synchronize()
    assert dec.__dict__.get("bad_labels") is not None and float(dec.bad_labels) == 0.0
    ts = []
    for loss, ce, i, weight in zip(ls, plain, (5, 4, 3, 2), (0.4, 0.6, 0.8, 1.0)):
        low = dec._taps["linear%d" % i].t.detach().cpu().numpy()
        r = R.ohem_ref(low, labn, ohem[0], ohem[1], False)
        ts.append(r.t)
        e_loss = abs(float(loss) - float(r.loss)) / float(r.loss)
        e_b = relmax(getattr(dec, "linear%d" % i).bias.grad.cpu().numpy(), r.dlow.sum((0, 1, 2)).numpy() * weight)
        print("linear%d: ohem loss %.6f (plain %.6f), %.3e rel; t %.6g; margin %.3e; bias gradient %.3e relmax" % (i, float(loss), ce, e_loss, r.t, r.margin, e_b))
        assert ohem[1] <= r.n_kept < ohem[1] + 8 and e_loss < LOSS_BAR and e_b < GRAD_BAR, (i, e_loss, e_b)
        assert float(loss) > ce
    assert len(set(ts)) == 4          # every head found its own threshold
    T = 1.8
    one = dec.loss(x, feats, lab, temperature=T, ohem=ohem)
    torch.cuda.synchronize()
    low2 = dec.last_low.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    r = R.ohem_ref(low2 / T, labn, ohem[0], ohem[1], False)
    e_loss = abs(float(one) - float(r.loss)) / float(r.loss)
    print("loss(): %.6f, %.3e rel; margin %.3e" % (float(one), e_loss, r.margin))
    assert e_loss < LOSS_BAR


def _cfg(tmp_path, *opts):
    from rnd_semantic_segmentation_amd.host import config as hc
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "MODEL.NUM_CLASSES", 19, "MODEL.FREEZE_BN", True, "SOLVER.EPOCHS", 1, "SOLVER.BASE_LR", 1e-4] + list(opts))
    cfg.freeze()
    return cfg


OHEM = ["SOLVER.LOSS", "ohem", "SOLVER.OHEM_THRESH", 0.02, "SOLVER.OHEM_MIN_KEPT", 700]


def test_aspp_trainer_step_with_the_loss_set_and_at_the_defaults(K, tmp_path):
    from rnd_semantic_segmentation_amd.host import modules
    from rnd_semantic_segmentation_amd.host.trainer import ASPPTrainer

    class Tiny(ASPPTrainer):
        build_feature_extractor = staticmethod(lambda cfg: modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False,
                                                                                            layers=(1, 1, 2, 2)))

    x, lab = _cases.net_inputs(2, 65, 11)
    xt, lt = torch.from_numpy(x), torch.from_numpy(lab)

    def make(*opts):
        tr = Tiny("aspp", _cfg(tmp_path, *opts), [None] * 50, 0, logger=logging.getLogger("ohem-aspp"))
        with torch.no_grad():
            for m in (tr.feature_extractor, tr.classifier):
                synth.load_formula_weights(m)
                m._store.generation += 1
        return tr

    tr = make(*OHEM)
    assert tr.ohem == (0.02, 700) and tr.ce_kwargs == {"ohem": (0.02, 700)}
    before = tr.classifier._store.data.clone()
    loss, _ = tr.train_step(xt, lt, 40)
    plain = make()
    assert plain.ce_kwargs == {} and plain.ohem is None
    loss0, _ = plain.train_step(xt, lt, 40)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and not torch.equal(before, tr.classifier._store.data)
    assert float(loss) > float(loss0)
    # the keys absent: the loss bits of this tree's default path
    other = make()
    want = other.classifier.loss(other.feature_extractor(xt.cuda()), lt.cuda().long(), 255)
    torch.cuda.synchronize()
    assert torch.equal(loss0, want.detach())
    # the mining step is classifier.loss with the helper's pair
    again = make(*OHEM)
    want_o = again.classifier.loss(again.feature_extractor(xt.cuda()), lt.cuda().long(), 255, ohem=(0.02, 700))
    torch.cuda.synchronize()
    assert torch.equal(loss, want_o.detach())
    kept = float(again.classifier._engine.last_loss_out[1])
    assert 700 <= kept < float((lab != 255).sum())


def test_gald_trainer_step_with_the_loss_set_and_at_the_defaults(K, tmp_path):
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()

    def make(*opts):
        log = logging.getLogger("ohem-gald")
        log.addHandler(logging.NullHandler())
        torch.manual_seed(11)
        tr = gald.GALDTrainer("gald", _cfg(tmp_path, *opts), None, 0, logger=log)
        tr.encoder.train()
        tr.decoder.train()
        return tr

    tr = make(*OHEM)
    assert tr.loss_name == "ohem" and tr.ohem == (0.02, 700)
    before = tr.decoder._store.data.clone()
    loss, _ = tr.train_step(x, lab, 100)
    plain = make()
    loss0, _ = plain.train_step(x, lab, 100)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and not torch.equal(before, tr.decoder._store.data)
    assert gald.take_bad_labels(tr.decoder, tr.criterion) == 0
    assert float(loss) > float(loss0)
    other = make()
    l5, l4, l3, l2 = other.decoder.losses(x, other.encoder(x), lab, criterion="ce")
    want = l2 * 1 + l3 * 0.8 + l4 * 0.6 + l5 * 0.4
    torch.cuda.synchronize()
    assert torch.equal(loss0, want.detach())
    again = make(*OHEM)
    l5, l4, l3, l2 = again.decoder.losses(x, again.encoder(x), lab, criterion="ohem", ohem=(0.02, 700))
    want_o = l2 * 1 + l3 * 0.8 + l4 * 0.6 + l5 * 0.4
    torch.cuda.synchronize()
    assert torch.equal(loss, want_o.detach())
