"""GPU tests of the fused upsample + generalized Dice loss (mi_upsample_gdl, csrc/upsample_ce.hip) and the layers above it: K.upsample_gdl against
the float64 restatement (tests/_gdl_ref.py) and the reference's own results (g16_gdl), its properties (bit-reproducible, loss-only, all-ignored,
out-of-range labels, tiny shapes, several rows and column tiles per workgroup, graph capture), metrics.GeneralizedDiceLoss, the GALD decoder's
criterion="gdl" heads and GALDTrainer with SOLVER.LOSS gdl.

Bars: those of upsample_ce in tests/test_gpu_ops.py - loss 2e-5 relative, dlow 2e-5 of the expectation's largest magnitude (scale-free: the 1e-12
gradients of the absent-class case are held to it too); the label histogram and the counts exactly."""
import functools
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gdl_ref as G
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

LOSS_BAR, GRAD_BAR = 2e-5, 2e-5


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g16_gdl.npz"))


def relmax(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(low, labels, float64 restatement) of a g16_gdl case: computed once, shared by the tests, never written to."""
    case = G.CASE_BY_NAME[name]
    low, lab = G.case_inputs(case)
    return low, lab, G.gdl_ref(low, lab, case.align_corners, case.weight_type)


def fused(K, low, lab, align_corners, weight_type="square", want_grad=True, **kw):
    """K.upsample_gdl on numpy NCHW logits -> (loss_out [4] numpy, dlow NCHW numpy or None, sums numpy)."""
    nhwc = torch.from_numpy(np.ascontiguousarray(low)).permute(0, 2, 3, 1).contiguous().cuda()
    out, dlow, sums = K.upsample_gdl(nhwc, torch.from_numpy(lab).cuda(), want_grad=want_grad, weight_type=weight_type, align_corners=align_corners,
                                     want_sums=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if dlow is None else dlow.permute(0, 3, 1, 2).cpu().numpy(), sums.cpu().numpy()


def check_against(r, out, dlow, sums, K_, lab, what):
    """loss_out / dlow / sums of one fused call against a restatement result `r`."""
    valid = (lab >= 0) & (lab < K_) & (lab != 255)
    assert np.array_equal(sums[:K_], np.bincount(lab[valid], minlength=K_).astype(np.float32)), what
    assert out[1] == float(valid.sum()) == float(r.valid) and out[2] == float(r.bad) and out[3] == 0.0, (what, out)
    assert np.isfinite(out).all() and np.isfinite(dlow).all() and np.isfinite(sums).all(), what
    e_loss = abs(float(out[0]) - float(r.loss)) / abs(float(r.loss))
    e_i = np.abs(sums[K_:2 * K_] - r.I.numpy()).max() / max(float(r.I.max()), 1e-30)
    e_p = np.abs(sums[2 * K_:] - r.P2.numpy()).max() / max(float(r.P2.max()), 1e-30)
    e_d = relmax(dlow, r.dlow.numpy()) if float(r.dlow.abs().max()) > 0 else float(np.abs(dlow).max())
    print("%s: loss %.3e rel, I %.3e, P2 %.3e, dlow %.3e relmax" % (what, e_loss, e_i, e_p, e_d))
    assert e_loss < LOSS_BAR and e_i < LOSS_BAR and e_p < LOSS_BAR and e_d < GRAD_BAR, (what, e_loss, e_i, e_p, e_d)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_parity_with_the_restatement_and_the_reference(K, golden, case):
    low, lab, r = case_ref(case.name)
    out, dlow, sums = fused(K, low, lab, case.align_corners, case.weight_type)
    want_loss, want_d = float(golden[case.name + ".loss"]), golden[case.name + ".dlow"]
    if case.name == "f":          # every pixel ignored: exactly 1, exactly zero, nothing NaN
        assert out[0] == 1.0 and out[1] == 0.0 and out[2] == 0.0 and want_loss == 1.0
        assert not dlow.any() and np.isfinite(dlow).all() and not sums.any()
        return
    check_against(r, out, dlow, sums, case.K, lab, case.name)
    e_loss, e_d = abs(float(out[0]) - want_loss) / abs(want_loss), relmax(dlow, want_d)
    print("%s vs the reference's fp32 run: loss %.3e rel, dlow %.3e relmax" % (case.name, e_loss, e_d))
    assert e_loss < LOSS_BAR and e_d < GRAD_BAR, (e_loss, e_d)


def test_two_calls_are_bit_equal_and_loss_only_gives_the_same_bits(K):
    for name in ("b_square", "e_ac"):
        case = G.CASE_BY_NAME[name]
        low, lab, _ = case_ref(name)
        a, b = fused(K, low, lab, case.align_corners, case.weight_type), fused(K, low, lab, case.align_corners, case.weight_type)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        out, dlow, sums = fused(K, low, lab, case.align_corners, case.weight_type, want_grad=False)
        assert dlow is None and out.tobytes() == a[0].tobytes() and sums.tobytes() == a[2].tobytes()


def test_out_of_range_labels_are_left_out_and_counted(K):
    case = G.CASE_BY_NAME["b_square"]
    low, lab, _ = case_ref("b_square")
    bad = lab.copy()
    bad.reshape(-1)[[3, 500, 501, 4000, 10529]] = [19, 254, -1, 1000, 2 ** 40]
    r = G.gdl_ref(low, bad, case.align_corners)
    assert r.bad == 5
    out, dlow, sums = fused(K, low, bad, case.align_corners)
    assert out[2] == 5.0
    check_against(r, out, dlow, sums, case.K, bad, "five bad labels")
    as_ignored = bad.copy()
    as_ignored[(bad < 0) | (bad >= 19)] = 255
    same = fused(K, low, as_ignored, case.align_corners)
    assert same[0][0].tobytes() == out[0].tobytes() and same[1].tobytes() == dlow.tobytes()


@pytest.mark.parametrize("B,Kc,hw,HW,align", [
    (1, 3, (1, 1), (1, 1), False), (2, 3, (1, 1), (5, 3), False), (1, 3, (1, 1), (5, 3), True), (1, 4, (2, 2), (2, 2), False),
    (1, 4, (2, 2), (2, 2), True), (2, 1, (2, 3), (4, 6), False), (1, 32, (3, 2), (7, 5), False),
    # several rows per workgroup and several column tiles, the last one partial (1 x 300 x 2000: 2400 row tiles -> 3 rows per workgroup)
    (1, 3, (10, 40), (300, 2000), False), (1, 19, (300, 520), (300, 520), True)])
def test_tiny_and_tiled_shapes_match_the_restatement(K, B, Kc, hw, HW, align):
    key = "g16.shape.%d.%d.%dx%d.%dx%d" % (B, Kc, hw[0], hw[1], HW[0], HW[1])
    low = (synth.uniform(key + ".low", (B, Kc) + hw) * 6).astype(np.float32)
    n = B * HW[0] * HW[1]
    lab = (synth.hash_u32(key + ".lab", n) % np.uint64(Kc)).astype(np.int64)
    if n > 8:
        lab[(synth.hash_u32(key + ".ign", n) % np.uint64(10)) == 0] = 255
    lab = lab.reshape((B,) + HW)
    for wt in (("square", "identity", "sqrt") if n < 100 else ("square",)):
        r = G.gdl_ref(low, lab, align, wt)
        out, dlow, sums = fused(K, low, lab, align, wt)
        check_against(r, out, dlow, sums, Kc, lab, "%s %s" % (key, wt))


def test_the_call_is_capturable_in_a_graph(K):
    case = G.CASE_BY_NAME["b_square"]
    low, lab, r = case_ref("b_square")
    nhwc = torch.from_numpy(low).permute(0, 2, 3, 1).contiguous().cuda()
    labc = torch.from_numpy(lab).cuda()
    src = torch.zeros_like(nhwc)
    K.upsample_gdl(src, labc, align_corners=False)          # first call outside the capture: code objects loaded, LDS attribute set
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, dlow, _ = K.upsample_gdl(src, labc, align_corners=False)
    src.copy_(nhwc)
    graph.replay()
    torch.cuda.synchronize()
    eager_out, eager_d, _ = K.upsample_gdl(nhwc, labc, align_corners=False)
    torch.cuda.synchronize()
    assert torch.equal(out, eager_out) and torch.equal(dlow, eager_d)
    assert abs(float(out[0]) - float(r.loss)) < LOSS_BAR * float(r.loss)


def test_generalized_dice_loss_on_materialised_logits(K):
    """metrics.GeneralizedDiceLoss (the reference's import path) on the materialised upsample of case (b) with .backward(), against the fused call on
    `low` (the gradient transposed through torch's bilinear), and `target` left as it is."""
    from core.utils.utility import GeneralizedDiceLoss
    case = G.CASE_BY_NAME["b_sqrt"]
    low, lab, r = case_ref("b_sqrt")
    out, dlow, _ = fused(K, low, lab, False, "sqrt")
    lowc = torch.from_numpy(low).cuda().requires_grad_(True)
    labc = torch.from_numpy(lab).cuda()
    keep = labc.clone()
    up = F.interpolate(lowc, size=case.HW, mode="bilinear", align_corners=False)
    loss, counts = GeneralizedDiceLoss(up, labc, weight_type="sqrt", with_counts=True)
    loss.backward()
    torch.cuda.synchronize()
    loss = loss.detach()
    assert torch.equal(labc, keep)
    assert not counts.requires_grad and float(counts[0]) == float(loss) and float(counts[1]) == float((labc != 255).sum()) and float(counts[2]) == 0.0
    e_loss, e_d = abs(float(loss) - float(out[0])) / float(out[0]), relmax(lowc.grad.cpu().numpy(), dlow)
    print("materialised vs fused: loss %.3e rel, dlow %.3e relmax" % (e_loss, e_d))
    assert e_loss < LOSS_BAR and e_d < GRAD_BAR
    assert abs(float(loss) - float(r.loss)) < LOSS_BAR * float(r.loss) and relmax(lowc.grad.cpu().numpy(), r.dlow.numpy()) < GRAD_BAR
    with torch.no_grad():
        assert float(GeneralizedDiceLoss(up.detach(), labc, weight_type="sqrt")) == float(loss)


# ------------------------------------------------------------------------------------------------ the GALD model
def _gald_inputs():
    x = torch.from_numpy(synth.synth_image(2, 224, 224, seed=5)).cuda()
    lab = torch.from_numpy(synth.synth_label(2, 224, 224, 19, seed=5)).long().cuda()
    return x, lab


def test_decoder_dice_heads_match_the_restatement_on_their_own_logits(K):
    """GCPAEncoder + GCPADecoder, 2 x 3 x 224 x 224, criterion="gdl": each of the four losses equals the restatement on the tapped low-resolution
    logits (linear5 .. linear2), and after backward each head's bias gradient equals the restatement's dlow summed over B, h, w and weighted
    0.4 / 0.6 / 0.8 / 1.  (The heads' logits and their gradients are fp32 on the tape and the bias gradient is summed from the fp32 gradient, so the
    expectation is not rounded to bf16.)"""
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()
    torch.manual_seed(3)
    enc, dec = gald.GCPAEncoder().cuda().train(), gald.GCPADecoder().cuda().train()
    with torch.no_grad():
        dec.long_relation.gamma.fill_(0.3)
    dec._taps = {}
    ls = dec.losses(x, enc(x), lab, criterion="gdl", weight_type="identity")
    (ls[3] * 1 + ls[2] * 0.8 + ls[1] * 0.6 + ls[0] * 0.4).backward()
    torch.cuda.synchronize()
    assert dec.__dict__.get("bad_labels") is not None and float(dec.bad_labels) == 0.0
    labn = lab.cpu().numpy()
    for loss, i, weight in zip(ls, (5, 4, 3, 2), (0.4, 0.6, 0.8, 1.0)):
        low = dec._taps["linear%d" % i].t.detach().permute(0, 3, 1, 2).cpu().numpy()
        r = G.gdl_ref(low, labn, False, "identity")
        e_loss = abs(float(loss) - float(r.loss)) / float(r.loss)
        want = r.dlow.sum((0, 2, 3)).numpy() * weight
        e_b = relmax(getattr(dec, "linear%d" % i).bias.grad.cpu().numpy(), want)
        print("linear%d: loss %.6f, %.3e rel; bias gradient %.3e relmax" % (i, float(loss), e_loss, e_b))
        assert e_loss < LOSS_BAR and e_b < GRAD_BAR, (i, e_loss, e_b)


def _trainer(tmp_path, *opts):
    from rnd_semantic_segmentation_amd.host import config as hc, gald
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "MODEL.NUM_CLASSES", 19, "SOLVER.EPOCHS", 1, "SOLVER.BASE_LR", 1e-4] + list(opts))
    cfg.freeze()
    log = logging.getLogger("gald_gdl")
    log.addHandler(logging.NullHandler())
    torch.manual_seed(11)
    tr = gald.GALDTrainer("gald", cfg, None, 0, logger=log)
    tr.encoder.train()
    tr.decoder.train()
    return tr


def _params(tr):
    return torch.cat([tr.encoder._store.data, tr.decoder._store.data]).clone()


def test_trainer_step_with_the_dice_loss(K, tmp_path):
    from rnd_semantic_segmentation_amd.host import gald
    x, lab = _gald_inputs()
    runs = []
    for _ in range(2):
        tr = _trainer(tmp_path, "SOLVER.LOSS", "gdl", "SOLVER.GDL_WEIGHT", "sqrt")
        assert tr.loss_name == "gdl" and tr.gdl_weight == "sqrt"
        before = _params(tr)
        loss, _ = tr.train_step(x, lab, 100)
        torch.cuda.synchronize()
        after = _params(tr)
        assert np.isfinite(float(loss)) and 0.0 < float(loss) < 2.8 and not torch.equal(before, after)
        assert gald.take_bad_labels(tr.decoder, tr.criterion) == 0
        runs.append((loss.clone(), after))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])          # bit-equal when repeated from the same state


def test_default_config_still_trains_with_cross_entropy(K, tmp_path):
    """SOLVER.LOSS defaults to "ce": the trainer's step gives the loss bits of decoder.losses(criterion="ce") in this same tree.  That proves the
    routing - the default config reaches the cross-entropy heads and nothing of the Dice path - and no more: that those heads compute what they
    did before the key existed rests on the cross-entropy tests of test_gpu_gald.py / test_gpu_ops.py, which this change leaves as they were."""
    x, lab = _gald_inputs()
    tr = _trainer(tmp_path)
    assert tr.loss_name == "ce"
    loss, _ = tr.train_step(x, lab, 100)
    other = _trainer(tmp_path)
    l5, l4, l3, l2 = other.decoder.losses(x, other.encoder(x), lab, criterion="ce")
    want = l2 * 1 + l3 * 0.8 + l4 * 0.6 + l5 * 0.4
    torch.cuda.synchronize()
    assert torch.equal(loss, want.detach())
