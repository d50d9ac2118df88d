"""GPU tests of the fused upsample + Tversky + BCE loss (mi_upsample_tversky_bce, csrc/upsample_ce.hip) and the layers above it:
K.upsample_tversky_bce against the float64 restatement (tests/_tversky_ref.py) and the reference's own results (g17_tversky), its properties
(bit-reproducible, loss-only, capturable in a graph), the loss modules at the reference's import path, PraNet.losses and PraNetTrainer with
SOLVER.LOSS tversky.

Bars: the project's own for fused upsample losses (tests/test_gpu_ops.py, tests/test_gpu_gdl.py) - loss, its two terms and TP / FN / FP 2e-5
relative, dlow 2e-5 of the expectation's largest magnitude."""
import functools
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _tversky_ref as T
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
    return np.load(os.path.join(golden_dir, "g17_tversky.npz"))


def relmax(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


def rel(got, want):
    got, want = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, want))
    return abs(got - want) if want == 0.0 else abs(got - want) / abs(want)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """(low, mask, float64 restatement) of a g17_tversky case: computed once, shared by the tests, never written to."""
    case = T.CASE_BY_NAME[name]
    low, mask = T.case_inputs(case)
    return low, mask, T.tversky_ref(low, mask, case.align_corners)


def fused(K, low, mask, align_corners=False, want_grad=True, **kw):
    """K.upsample_tversky_bce on numpy operands -> (loss_out [4] numpy, dlow numpy or None, sums numpy)."""
    out, dlow, sums = K.upsample_tversky_bce(torch.from_numpy(low).cuda(), torch.from_numpy(mask).cuda(), want_grad=want_grad, align_corners=align_corners,
                                             want_sums=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if dlow is None else dlow.cpu().numpy(), sums.cpu().numpy()


def check_against(r, out, dlow, sums, what):
    """loss_out / dlow / sums of one fused call against a restatement result `r`."""
    assert np.isfinite(out).all() and np.isfinite(dlow).all() and np.isfinite(sums).all() and out[3] == 0.0, what
    errs = [rel(out[0], r.loss), rel(out[1], r.tversky), rel(out[2], r.bce), rel(sums[0], r.TP), rel(sums[1], r.FN), rel(sums[2], r.FP)]
    e_d = relmax(dlow, r.dlow.numpy())
    print("%s: loss %.3e, tversky %.3e, bce %.3e, TP %.3e, FN %.3e, FP %.3e rel; dlow %.3e relmax" % tuple([what] + errs + [e_d]))
    assert max(errs) < LOSS_BAR and e_d < GRAD_BAR, (what, errs, e_d)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_parity_with_the_restatement_and_the_reference(K, golden, case):
    low, mask, r = case_ref(case.name)
    out, dlow, sums = fused(K, low, mask, case.align_corners)
    check_against(r, out, dlow, sums, case.name)
    want_d = golden[case.name + ".dlow"]
    errs = [rel(out[0], golden[case.name + ".loss"]), rel(out[1], golden[case.name + ".tversky"]), rel(out[2], golden[case.name + ".bce"])]
    e_d = relmax(dlow, want_d)
    print("%s vs the reference's fp32 run: loss %.3e, tversky %.3e, bce %.3e rel; dlow %.3e relmax" % tuple([case.name] + errs + [e_d]))
    assert max(errs) < LOSS_BAR and e_d < GRAD_BAR, (errs, e_d)
    if case.mask == "zero":
        assert sums[0] == 0.0 and sums[1] == 0.0 and sums[2] > 0.0
    if case.mask == "one":
        assert sums[2] == 0.0 and sums[0] > 0.0
    if case.sat:
        assert out[0] > 2.0


def test_alpha_and_weights(K):
    """alpha 0.3 and either term alone on case (c); the BCE alone also equals F.binary_cross_entropy_with_logits on torch's upsample."""
    case = T.CASE_BY_NAME["c"]
    low, mask, _ = case_ref("c")
    for alpha, weights in ((0.3, (0.5, 0.5)), (0.3, (1.0, 0.0)), (0.7, (0.0, 1.0))):
        r = T.tversky_ref(low, mask, False, alpha=alpha, weights=weights)
        out, dlow, sums = fused(K, low, mask, False, alpha=alpha, weights=weights)
        check_against(r, out, dlow, sums, "c alpha %g weights %s" % (alpha, weights))
    lowc = torch.from_numpy(low).cuda().unsqueeze(1).requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(F.interpolate(lowc, size=case.HW, mode="bilinear", align_corners=False), torch.from_numpy(mask).cuda().unsqueeze(1))
    want.backward()
    e_loss, e_d = rel(out[0], want), relmax(dlow, lowc.grad[:, 0].cpu().numpy())
    print("bce alone vs torch: loss %.3e rel, dlow %.3e relmax" % (e_loss, e_d))
    assert out[0] == out[2] and e_loss < LOSS_BAR and e_d < GRAD_BAR


@pytest.mark.parametrize("B,hw,HW,align", T.TILED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tiny_and_tiled_shapes_match_the_restatement(K, B, hw, HW, align):
    """No grid of the entry is capped (one workgroup per tile in all three launches); the finalize's loop over the partial rows takes its second trip
    from 257 workgroups on, which the three 352 x 352 shapes have (704)."""
    key = "g17.shape.%d.%dx%d.%dx%d" % (B, hw[0], hw[1], HW[0], HW[1])
    low, mask = T.make_inputs(key, B, hw, HW, "soft" if hw[0] == 22 else "hard")
    r = T.tversky_ref(low, mask, align)
    out, dlow, sums = fused(K, low, mask, align)
    check_against(r, out, dlow, sums, key)


def test_two_calls_are_bit_equal_and_loss_only_gives_the_same_bits(K):
    for name in ("b", "i"):
        case = T.CASE_BY_NAME[name]
        low, mask, _ = case_ref(name)
        a, b = fused(K, low, mask, case.align_corners), fused(K, low, mask, case.align_corners)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        out, dlow, sums = fused(K, low, mask, case.align_corners, want_grad=False)
        assert dlow is None and out.tobytes() == a[0].tobytes() and sums.tobytes() == a[2].tobytes()


def test_the_call_is_capturable_in_a_graph(K):
    low, mask, r = case_ref("g")
    lowc, maskc = torch.from_numpy(low).cuda(), torch.from_numpy(mask).cuda()
    src = torch.zeros_like(lowc)
    K.upsample_tversky_bce(src, maskc)          # first call outside the capture: code objects loaded, workspace allocated
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, dlow, _ = K.upsample_tversky_bce(src, maskc)
    src.copy_(lowc)
    graph.replay()
    torch.cuda.synchronize()
    eager_out, eager_d, _ = K.upsample_tversky_bce(lowc, maskc)
    torch.cuda.synchronize()
    assert torch.equal(out, eager_out) and torch.equal(dlow, eager_d)
    assert rel(out[0], r.loss) < LOSS_BAR


def test_loss_modules_on_a_materialised_upsample(K, monkeypatch):
    """The modules at the reference's import path on the materialised upsample of case (g) with .backward(), against the fused call on `low` (the
    gradient transposed through torch's bilinear); the mask is left as it is; the compound of both terms is ONE kernel call."""
    from core.models.classifiers.attn.loss import BinaryCrossEntropyLoss, CompoundLoss, MultiscaleLoss, TverskyLoss
    case = T.CASE_BY_NAME["g"]
    low, mask, r = case_ref("g")
    calls = []
    real = K.upsample_tversky_bce
    monkeypatch.setattr(K, "upsample_tversky_bce", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    maskc = torch.from_numpy(mask).cuda().unsqueeze(1)
    keep = maskc.clone()
    for crit, weights in ((CompoundLoss([TverskyLoss(), BinaryCrossEntropyLoss()]), (0.5, 0.5)), (TverskyLoss(alpha=0.3), (1.0, 0.0)),
                          (BinaryCrossEntropyLoss(), (0.0, 1.0)), (CompoundLoss([TverskyLoss(), BinaryCrossEntropyLoss()], weights=[0.25, 2.0]), (0.25, 2.0))):
        alpha = 0.3 if weights == (1.0, 0.0) else 0.7
        del calls[:]
        out, dlow, _ = fused(K, low, mask, False, alpha=alpha, weights=weights)
        assert len(calls) == 1
        lowc = torch.from_numpy(low).cuda().unsqueeze(1).requires_grad_(True)
        up = F.interpolate(lowc, size=case.HW, mode="bilinear", align_corners=False)
        loss = crit(up, maskc)
        assert len(calls) == 2, "one kernel call per criterion, the compound included"
        loss.backward()
        torch.cuda.synchronize()
        assert torch.equal(maskc, keep)
        got_d = lowc.grad[:, 0].cpu().numpy()
        e_loss, e_d = rel(loss, out[0]), relmax(got_d, dlow)
        print("%s: materialised vs fused: loss %.3e rel, dlow %.3e relmax" % (type(crit).__name__, e_loss, e_d))
        assert e_loss < LOSS_BAR and e_d < GRAD_BAR
        want = T.tversky_ref(low, mask, False, alpha=alpha, weights=weights)
        assert rel(loss, want.loss) < LOSS_BAR and relmax(got_d, want.dlow.numpy()) < GRAD_BAR
    # [B,H,W] operands and the multi-scale sum: two heads, the terms added up
    multi = MultiscaleLoss(CompoundLoss([TverskyLoss(), BinaryCrossEntropyLoss()]))
    p3 = F.interpolate(torch.from_numpy(low).cuda().unsqueeze(1), size=case.HW, mode="bilinear", align_corners=False)[:, 0].contiguous()
    total = multi([p3, p3.unsqueeze(1)], [maskc[:, 0], maskc])
    assert rel(total, 2.0 * float(r.loss)) < LOSS_BAR
    with pytest.raises(NotImplementedError, match="C > 1"):
        TverskyLoss()(torch.zeros(2, 3, 4, 5).cuda(), torch.zeros(2, 3, 4, 5).cuda())


# ------------------------------------------------------------------------------------------------ the PraNet model
def _pranet_inputs(B=2, S=160):
    img, mask = synth.synth_polyp(B, S, S, seed=21)
    return torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()


def _fresh_net(seed=5):
    from rnd_semantic_segmentation_amd.host import pranet
    torch.manual_seed(seed)
    net = pranet.PraNet().cuda().train()
    net.ensure_flat()
    return net


def test_pranet_heads_match_the_restatement_on_their_own_maps(K):
    """PraNet, 2 x 3 x 160 x 160, train mode: each of the four PraNet.losses values equals the restatement on the tapped low-resolution map (coarse, ra4,
    ra3, ra2), and after backward of their sum the BatchNorm bias gradient of ra2_conv4 - the last unit of the one branch whose map feeds nothing but its
    head - equals the restatement's dlow summed over B, h, w.  (The side maps and their gradients are fp32 on the tape and the bias gradient is summed
    from the fp32 gradient, so the expectation is not rounded to bf16.)"""
    x, gt = _pranet_inputs()
    net = _fresh_net()
    net._taps = {}
    ls = net.losses(x, gt)
    (ls[3] + ls[2] + ls[1] + ls[0]).backward()
    torch.cuda.synchronize()
    assert net.__dict__.get("_tversky") is None and not any(k.startswith("map") for k in net._taps)
    maskn = gt.cpu().numpy()
    for loss, name, factor in zip(ls, ("coarse", "ra4", "ra3", "ra2"), (8, 32, 16, 8)):
        low = net._taps[name].t.detach()
        assert low.dtype == torch.float32 and tuple(low.shape) == (2, 160 // factor, 160 // factor, 1)
        r = T.tversky_ref(low[..., 0].cpu().numpy(), maskn, False)
        e_loss = rel(loss, r.loss)
        print("%s: loss %.6f, %.3e rel" % (name, float(loss.detach()), e_loss))
        assert e_loss < LOSS_BAR, (name, e_loss)
    got, want = float(net.ra2_conv4.bn.bias.grad), float(r.dlow.sum())
    print("ra2_conv4.bn.bias.grad %.9g vs sum dlow2 %.9g: %.3e rel" % (got, want, rel(got, want)))
    assert rel(got, want) < GRAD_BAR


def _flat_grad(net):
    return net._store.grad.detach().double().clone()


def _cos_and_norm(a, b):
    return 1.0 - float(torch.dot(a, b) / (a.norm() * b.norm())), abs(float(a.norm() / b.norm()) - 1.0)


def test_fused_heads_against_the_literal_composition(K):
    """Fused heads (PraNet.losses) against the literal composition (net(x) -> the host/losses.py modules) in the same tree, 2 x 3 x 160 x 160: the four
    losses agree at the loss bar; the flat parameter gradients differ by fp32 rounding in dlow that the bf16 backward then amplifies.
    Yardstick: the structure-loss step through run.resize against itself with its four map gradients perturbed by a relative 2e-5 (two sign patterns);
    the bar on 1 - cos and on the norm ratio is 3 x the larger of the yardstick's two values, and never above the conditioned-regime ceilings of
    tests/test_gpu_pranet.py (1 - cos 0.05, norm 0.1).
    Measured (MI355X): fused against literal 1 - cos below 1e-15 (printed as -2.2e-16), norm ratio off by 4.9e-15 - the fp32 rounding differences in dlow
    (4e-7) almost never survive the first bf16 rounding of the backward pass; yardstick 1 - cos 2.47e-4 / 2.71e-4, norm 1.73e-3 / 5.6e-5, hence
    bars of 8.1e-4 and 5.2e-3."""
    from rnd_semantic_segmentation_amd.host import pranet
    x, gt = _pranet_inputs()

    def grads(losses_of=None, map_grads=None):
        net = _fresh_net()
        net.zero_grad()
        if map_grads is None:
            ls = losses_of(net)
            (ls[3] + ls[2] + ls[1] + ls[0]).backward()
        else:
            ls = None
            torch.autograd.backward(list(net(x)), map_grads)
        torch.cuda.synchronize()
        return ls, _flat_grad(net)

    fused_ls, g_fused = grads(lambda net: pranet.step_losses(net, x, gt, "tversky"))
    lit_ls, g_lit = grads(lambda net: pranet.step_losses(net, x, gt, "tversky", literal=True))
    for a, b in zip(fused_ls, lit_ls):
        assert rel(a, b) < LOSS_BAR, (float(a), float(b))
    cos, norm = _cos_and_norm(g_fused, g_lit)
    # the yardstick: d structure_loss / d map for the four maps, handed to the tape as they are and perturbed
    net = _fresh_net()
    with torch.no_grad():
        exact = [K.structure_loss(o.float().contiguous(), gt)[1] for o in net(x)]
    _, g_exact = grads(map_grads=exact)
    yard = []
    for salt in (1, 2):
        pert = []
        for i, g in enumerate(exact):
            sign = torch.from_numpy(np.where(synth.hash_u32("g17.perturb%d" % i, g.numel(), salt=salt) % np.uint64(2), 1.0, -1.0).astype(np.float32)).cuda()
            pert.append(g * (1.0 + 2e-5 * sign.view_as(g)))
        yard.append(_cos_and_norm(grads(map_grads=pert)[1], g_exact))
    bar_cos, bar_norm = min(3.0 * max(y[0] for y in yard), 0.05), min(3.0 * max(y[1] for y in yard), 0.1)
    print("fused vs literal: 1 - cos %.3e, norm %.3e; yardstick (2e-5 on the map gradients): 1 - cos %.3e / %.3e, norm %.3e / %.3e; bars %.3e, %.3e"
          % (cos, norm, yard[0][0], yard[1][0], yard[0][1], yard[1][1], bar_cos, bar_norm))
    assert cos <= bar_cos and norm <= bar_norm, (cos, norm, yard)


def _trainer(tmp_path, *opts):
    from rnd_semantic_segmentation_amd.host import config as hc, pranet
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "SOLVER.EPOCHS", 1, "SOLVER.BASE_LR", 1e-4, "INPUT.TRAINSIZE", 160] + list(opts))
    cfg.freeze()
    log = logging.getLogger("pranet_tversky")
    log.addHandler(logging.NullHandler())
    torch.manual_seed(11)
    tr = pranet.PraNetTrainer("pranet", cfg, None, 0, logger=log)
    tr.model.train()
    return tr


def test_trainer_step_with_the_tversky_loss(K, tmp_path, monkeypatch):
    monkeypatch.setenv("MI_GRAPH", "0")
    x, gt = _pranet_inputs()
    runs = []
    for _ in range(2):
        tr = _trainer(tmp_path, "SOLVER.LOSS", "tversky", "SOLVER.TVERSKY_ALPHA", 0.6)
        assert tr.loss_name == "tversky" and tr.tversky_alpha == 0.6
        before = tr.model._store.data.clone()
        ls = tr.train_step(x, gt)
        torch.cuda.synchronize()
        after = tr.model._store.data.clone()
        assert len(ls) == 4 and all(np.isfinite(float(l)) and 0.0 < float(l) < 10.0 for l in ls) and not torch.equal(before, after)
        runs.append(([l.detach().clone() for l in ls], after))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])) and torch.equal(runs[0][1], runs[1][1])      # bit-equal from the same state
    other = _trainer(tmp_path, "SOLVER.LOSS", "tversky", "SOLVER.TVERSKY_ALPHA", 0.6)
    want = other.model.losses(x, gt, alpha=0.6)
    assert all(torch.equal(a, b.detach()) for a, b in zip(runs[0][0], want))


def test_tversky_graph_replay_is_bit_equal_to_eager(K, tmp_path, monkeypatch):
    """PraNetTrainer.train_step with SOLVER.LOSS tversky, MI_GRAPH off against on (three eager steps, then the captured step replayed), 2 x 3 x 96 x 96
    on changing inputs: identical losses after every step and identical parameters after five."""
    data = [synth.synth_polyp(2, 96, 96, seed=60 + i) for i in range(5)]

    def run(graph):
        monkeypatch.setenv("MI_GRAPH", "1" if graph else "0")
        tr = _trainer(tmp_path, "SOLVER.LOSS", "tversky", "INPUT.TRAINSIZE", 96)
        tr.optimizer.set_device_hyper(True)          # every step, eager or replayed, through the update kernel of the replay (as tests/test_gpu_pranet.py)
        out = []
        for img, mask in data:
            out.append([float(l) for l in tr.train_step(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda())])
        torch.cuda.synchronize()
        assert (tr.__dict__.get("_graph", {}).get("step") is not None) == graph
        return out, tr.model._store.data.clone()

    eager, p_eager = run(False)
    replayed, p_replayed = run(True)
    assert replayed == eager, (replayed, eager)
    assert torch.equal(p_eager, p_replayed)


def test_default_config_still_trains_with_the_structure_loss(K, tmp_path, monkeypatch):
    """SOLVER.LOSS defaults to "ce": the trainer's step gives the loss bits of the structure-loss path called directly in this same tree.  That proves
    the routing - the default config reaches the four materialised maps and nothing of the Tversky path - and no more: that this path computes what
    it did before the key existed rests on tests/test_gpu_pranet.py, which this change leaves as it was."""
    from rnd_semantic_segmentation_amd.host import pranet
    monkeypatch.setenv("MI_GRAPH", "0")
    x, gt = _pranet_inputs()
    tr = _trainer(tmp_path)
    assert tr.loss_name == "ce"
    ls = tr.train_step(x, gt)
    other = _trainer(tmp_path)
    want = [pranet.structure_loss(o, gt) for o in other.model(x)]
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(ls, want))
