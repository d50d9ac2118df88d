"""GPU tests of the boundary (signed-distance) loss: mi_signed_distance (csrc/signed_distance.hip) against the exhaustive d2 / phi of
tests/_sdf_ref.py - exact integers and equal bits -, mi_upsample_tversky_bce_sdf (csrc/upsample_ce.hip) against the float64 restatement,
losses.BoundaryLoss, and PraNet / PraNetTrainer with SOLVER.BOUNDARY_WEIGHT.

Bars.  d2: np.array_equal; phi: the bytes of float32(sqrt(float64(d2))) with the sign rule.  The head's Tversky / BCE parts, TP / FN / FP, the loss and
dlow: the bars of tests/test_gpu_tversky.py (2e-5 relative; dlow 2e-5 of the expectation's largest magnitude).  The boundary part and the combined
gradient in addition: at most SDF_FACTOR (16, the ratio of tests/test_gpu_crf.py) times what the same restatement run in float32 on the CPU
deviates from float64 on that case - computed here, not hard-coded.  Every test prints the figures it asserts on."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _sdf_ref as S
import _tversky_ref as T
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

LOSS_BAR, GRAD_BAR = 2e-5, 2e-5
SDF_FACTOR = 16.0


@pytest.fixture(scope="module")
def K():
    import __graft_entry__ as entry
    entry.build()
    from rnd_semantic_segmentation_amd import kernels
    return kernels


def rel(got, want):
    got, want = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, want))
    return abs(got - want) if want == 0.0 else abs(got - want) / abs(want)


def relmax(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / np.abs(want).max()


# ------------------------------------------------------------------------------------------------ mi_signed_distance
def _capped_grid_mask():
    """65535 x 1 x 17: 65535 rows and 17408 column workgroups, both above the 16384 workgroups a launch takes - every workgroup strides."""
    return (synth.uniform("sdf.cap", (65535, 1, 17)) > 0.2).astype(np.float32)


MASKS = {
    "2x5x7": lambda: S.blobs("sdf.a", 2, 5, 7),
    "1x37x70": lambda: S.blobs("sdf.b", 1, 37, 70),                       # W crosses a wave and is no multiple of 64
    "3x300x260": lambda: S.blobs("sdf.big", 3, 300, 260),                 # W > 256: a second trip of the x loop; H no multiple of 8
    "speckle": lambda: S.speckle("sdf.c", 2, 33, 45),
    "mixed": S.mixed_batch,                                               # empty, full, single pixels, checkerboard, two far blobs
    "soft": S.soft_mask,                                                  # exactly 0.5 and the float just below it
    "nan": S.nan_mask,
    "capped-grid": _capped_grid_mask,
}


@functools.lru_cache(maxsize=None)
def mask_ref(name):
    """(mask, d2, G, phi) of a case: computed once, shared, never written to."""
    mask = MASKS[name]()
    d2, G = S.d2_ref(mask)
    return mask, d2, G, S.phi_of(d2, G)


@pytest.mark.parametrize("name", list(MASKS))
def test_d2_is_exact_and_phi_is_bit_equal(K, name):
    mask, d2, G, phi = mask_ref(name)
    got_phi, got_d2, counts = K.signed_distance(torch.from_numpy(mask).cuda(), want_d2=True, want_counts=True)
    torch.cuda.synchronize()
    got_phi, got_d2, counts = got_phi.cpu().numpy(), got_d2.cpu().numpy(), counts.cpu().numpy()
    fg = G.reshape(G.shape[0], -1).sum(1)
    assert np.array_equal(counts[:, 0], fg) and np.array_equal(counts[:, 1], G[0].size - fg)
    print("%s: max d2 %d, %d of %d images without a contour" % (name, d2.max(), int(((fg == 0) | (fg == G[0].size)).sum()), G.shape[0]))
    assert got_d2.dtype == np.int32 and np.array_equal(got_d2, d2)
    assert got_phi.dtype == np.float32 and got_phi.tobytes() == phi.tobytes()
    if name == "mixed":
        assert not got_phi[0].any() and not got_phi[1].any() and got_d2[2, 0, -1] == 40 ** 2 + 66 ** 2          # the far corner of the single pixel


def test_threshold_and_plain_call(K):
    """thresh is honoured (a soft mask at 0.25 and 0.75), and the call without the diagnosis outputs returns the same phi."""
    mask = (synth.uniform("sdf.thr", (2, 21, 30)) + 0.5).astype(np.float32)
    m = torch.from_numpy(mask).cuda()
    for thresh in (0.25, 0.75):
        want = S.phi_ref(mask, thresh)
        phi = K.signed_distance(m, thresh)
        both = K.signed_distance(m, thresh, want_d2=True)
        assert phi.cpu().numpy().tobytes() == want.tobytes() and torch.equal(phi, both[0]) and both[2] is None


def test_two_calls_are_bit_equal_and_the_call_is_capturable(K):
    a, _, _, phi_a = mask_ref("3x300x260")
    b = np.ascontiguousarray(a[:, ::-1, :])
    buf = torch.from_numpy(a).cuda()
    first, second = K.signed_distance(buf, want_d2=True), K.signed_distance(buf, want_d2=True)          # (also: workspace allocated before the capture)
    torch.cuda.synchronize()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        phi = K.signed_distance(buf)
    graph.replay()
    torch.cuda.synchronize()
    assert phi.cpu().numpy().tobytes() == phi_a.tobytes()
    buf.copy_(torch.from_numpy(b).cuda())                 # the mask buffer changes: a replay gives the new map
    graph.replay()
    torch.cuda.synchronize()
    assert phi.cpu().numpy().tobytes() == np.ascontiguousarray(phi_a[:, ::-1, :]).tobytes()


# ------------------------------------------------------------------------------------------------ mi_upsample_tversky_bce_sdf
HEADS = {
    "2x11x13-44x52": dict(B=2, hw=(11, 13), HW=(44, 52), align=False, w_bd=0.01, empty=None),
    "2x11x13-44x52-align": dict(B=2, hw=(11, 13), HW=(44, 52), align=True, w_bd=0.01, empty=None),
    "identity-1x7x9": dict(B=1, hw=(7, 9), HW=(7, 9), align=False, w_bd=0.25, empty=None),
    "identity-1x7x9-align": dict(B=1, hw=(7, 9), HW=(7, 9), align=True, w_bd=0.25, empty=None),
    "tiled-2x11x11-352x352": dict(B=2, hw=(11, 11), HW=(352, 352), align=False, w_bd=0.01, empty=None),          # of _tversky_ref.TILED
    "phi0-image-3x6x5-48x40": dict(B=3, hw=(6, 5), HW=(48, 40), align=False, w_bd=0.05, empty=1),                # image 1 has no contour
}
assert (2, (11, 11), (352, 352), False) in T.TILED


@functools.lru_cache(maxsize=None)
def head_ref(name):
    """(low, mask, phi, float64 restatement, float32 restatement, Tversky / BCE restatement of _tversky_ref) of a head case."""
    c = HEADS[name]
    low, _ = T.make_inputs("sdf.head." + name, c["B"], c["hw"], c["HW"])
    mask = S.blobs("sdf.head." + name, c["B"], *c["HW"])
    if c["empty"] is not None:
        mask[c["empty"]] = 0.0
    phi = S.phi_ref(mask)
    r64 = S.sdf_loss_ref(low, mask, phi, c["align"], w_boundary=c["w_bd"])
    r32 = S.sdf_loss_ref(low, mask, phi, c["align"], w_boundary=c["w_bd"], dtype=torch.float32)
    return low, mask, phi, r64, r32, T.tversky_ref(low, mask, c["align"])


def fused(K, low, mask, phi, align, w_bd, want_grad=True):
    out, dlow, sums = K.upsample_tversky_bce(torch.from_numpy(low).cuda(), torch.from_numpy(mask).cuda(), want_grad=want_grad, align_corners=align,
                                             want_sums=True, phi=None if phi is None else torch.from_numpy(phi).cuda(), w_boundary=w_bd)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if dlow is None else dlow.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("name", list(HEADS))
def test_head_parity_with_the_float64_restatement(K, name):
    c = HEADS[name]
    low, mask, phi, r64, r32, tv = head_ref(name)
    if c["empty"] is not None:
        assert not phi[c["empty"]].any() and phi.any()
    out, dlow, sums = fused(K, low, mask, phi, c["align"], c["w_bd"])
    assert np.isfinite(out).all() and np.isfinite(dlow).all() and np.isfinite(sums).all()
    # the parts the plain entry has: its bars
    errs = [rel(out[0], r64.loss), rel(out[1], r64.tversky), rel(out[2], r64.bce), rel(out[1], tv.tversky), rel(out[2], tv.bce),
            rel(sums[0], tv.TP), rel(sums[1], tv.FN), rel(sums[2], tv.FP)]
    e_d = relmax(dlow, r64.dlow.numpy())
    print("%s: loss %.3e, tversky %.3e, bce %.3e (vs _tversky_ref %.3e, %.3e), TP %.3e, FN %.3e, FP %.3e rel; dlow %.3e relmax" % tuple([name] + errs + [e_d]))
    assert max(errs) < LOSS_BAR and e_d < GRAD_BAR, (errs, e_d)
    # the boundary part and the combined gradient against the float32 restatement's own deviation
    dev_b, err_b = abs(float(r32.boundary) - float(r64.boundary)), abs(float(out[3]) - float(r64.boundary))
    dev_s, err_s = abs(float(r32.S) - float(r64.S)), abs(float(sums[3]) - float(r64.S))
    dev_d, err_d = float((r32.dlow.double() - r64.dlow).abs().max()), float(np.abs(dlow.astype(np.float64) - r64.dlow.numpy()).max())
    print("%s: boundary %.9g: |kernel - f64| %.3e, float32 restatement %.3e, ratio %.2f; S ratio %.2f; dlow: %.3e against %.3e, ratio %.2f (bound %.0f)"
          % (name, float(r64.boundary), err_b, dev_b, err_b / dev_b if dev_b else float("inf") if err_b else 0.0, err_s / dev_s if dev_s else float("inf") if err_s else 0.0,
             err_d, dev_d, err_d / dev_d, SDF_FACTOR))
    assert err_b <= SDF_FACTOR * dev_b, (err_b, dev_b)
    assert err_d <= SDF_FACTOR * dev_d, (err_d, dev_d)


def test_zero_weight_matches_the_plain_entry_and_loss_only_gives_the_same_bits(K):
    """w_boundary = 0 with an arbitrary phi: loss_out[3] == 0 (the term is off), the loss and the gradient are the plain entry's within its bars (and
    the restatement's); loss-only gives the same loss bits; two calls are bit-equal."""
    for name in ("2x11x13-44x52", "identity-1x7x9-align"):
        c = HEADS[name]
        low, mask, phi, r64, _, tv = head_ref(name)
        arbitrary = (synth.uniform("sdf.arbitrary." + name, phi.shape) * 40.0).astype(np.float32)
        plain = fused(K, low, mask, None, c["align"], 0.0)
        zero = fused(K, low, mask, arbitrary, c["align"], 0.0)
        assert plain[0][3] == 0.0 and plain[2].shape == (3,) and zero[2].shape == (4,)
        e_loss, e_d = rel(zero[0][0], plain[0][0]), relmax(zero[1], plain[1])
        print("%s, w_boundary 0: loss %.3e rel, dlow %.3e relmax against the plain entry" % (name, e_loss, e_d))
        assert e_loss < LOSS_BAR and e_d < GRAD_BAR and rel(zero[0][0], tv.loss) < LOSS_BAR and relmax(zero[1], tv.dlow.numpy()) < GRAD_BAR
        assert zero[0][3] == 0.0 and np.isfinite(zero[2][3])
        a, b = fused(K, low, mask, phi, c["align"], c["w_bd"]), fused(K, low, mask, phi, c["align"], c["w_bd"])
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        out, dlow, sums = fused(K, low, mask, phi, c["align"], c["w_bd"], want_grad=False)
        assert dlow is None and out.tobytes() == a[0].tobytes() and sums.tobytes() == a[2].tobytes()
    with pytest.raises(ValueError, match="w_boundary"):
        K.upsample_tversky_bce(torch.zeros(1, 2, 2).cuda(), torch.zeros(1, 4, 4).cuda(), w_boundary=0.01)


# ------------------------------------------------------------------------------------------------ losses.BoundaryLoss
def test_boundary_loss_module_on_a_materialised_upsample(K):
    """BoundaryLoss alone and as the third term of a CompoundLoss, on the materialised upsample with .backward(), against the restatement (the gradient
    transposed through torch's bilinear)."""
    from rnd_semantic_segmentation_amd.host.losses import BinaryCrossEntropyLoss, BoundaryLoss, CompoundLoss, TverskyLoss
    name = "2x11x13-44x52"
    c = HEADS[name]
    low, mask, phi, r64, _, _ = head_ref(name)
    maskc = torch.from_numpy(mask).cuda().unsqueeze(1)
    keep = maskc.clone()
    only = S.sdf_loss_ref(low, mask, phi, c["align"], weights=(0.0, 0.0), w_boundary=1.0)
    for crit, want in ((BoundaryLoss(), only), (CompoundLoss([TverskyLoss(), BinaryCrossEntropyLoss(), BoundaryLoss()], weights=[0.5, 0.5, c["w_bd"]]), r64)):
        lowc = torch.from_numpy(low).cuda().unsqueeze(1).requires_grad_(True)
        loss = crit(F.interpolate(lowc, size=c["HW"], mode="bilinear", align_corners=c["align"]), maskc)
        loss.backward()
        torch.cuda.synchronize()
        e_loss, e_d = rel(loss, want.loss), relmax(lowc.grad[:, 0].cpu().numpy(), want.dlow.numpy())
        print("%s: loss %.9g, %.3e rel; dlow %.3e relmax" % (type(crit).__name__, float(loss.detach()), e_loss, e_d))
        assert e_loss < LOSS_BAR and e_d < GRAD_BAR and torch.equal(maskc, keep)
    with pytest.raises(NotImplementedError, match="C > 1"):
        BoundaryLoss()(torch.zeros(2, 3, 4, 5).cuda(), torch.zeros(2, 3, 4, 5).cuda())


# ------------------------------------------------------------------------------------------------ PraNet
def _pranet_inputs(B=2, size=160):
    img, mask = synth.synth_polyp(B, size, size, seed=21)
    return torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()


def _fresh_net(seed=5):
    from rnd_semantic_segmentation_amd.host import pranet
    torch.manual_seed(seed)
    net = pranet.PraNet().cuda().train()
    net.ensure_flat()
    return net


def _cos_and_norm(a, b):
    return 1.0 - float(torch.dot(a, b) / (a.norm() * b.norm())), abs(float(a.norm() / b.norm()) - 1.0)


def test_fused_heads_against_the_literal_composition(K, monkeypatch):
    """PraNet.losses with boundary_weight 0.01 against the literal composition (net(x) -> CompoundLoss([Tversky, BCE, BoundaryLoss])), 2 x 3 x 160 x 160,
    the shape and batch of tests/test_gpu_tversky.py's test of the same name and its bars: the four losses at the loss bar; 1 - cos and the norm ratio
    of the flat parameter gradients at 3 x the yardstick (the structure-loss step against itself with its four map gradients perturbed by a relative
    2e-5, two sign patterns), never above 0.05 / 0.1.  phi is computed once per fused step and shared by the four heads."""
    from rnd_semantic_segmentation_amd.host import pranet
    x, gt = _pranet_inputs()
    calls = []
    real = K.signed_distance
    monkeypatch.setattr(K, "signed_distance", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

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
        return ls, net._store.grad.detach().double().clone()

    fused_ls, g_fused = grads(lambda net: pranet.step_losses(net, x, gt, "tversky", boundary_weight=0.01))
    assert len(calls) == 1, "one distance map per step, shared by the four heads"
    lit_ls, g_lit = grads(lambda net: pranet.step_losses(net, x, gt, "tversky", literal=True, boundary_weight=0.01))
    plain_ls, _ = grads(lambda net: pranet.step_losses(net, x, gt, "tversky"))
    for a, b, p in zip(fused_ls, lit_ls, plain_ls):
        print("fused %.7f, literal %.7f (%.3e rel); without the term %.7f" % (float(a.detach()), float(b.detach()), rel(a, b), float(p.detach())))
        assert rel(a, b) < LOSS_BAR and abs(float(a.detach()) - float(p.detach())) > 1e-4, "the term is there"
    cos, norm = _cos_and_norm(g_fused, g_lit)
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
    print("fused vs literal: 1 - cos %.3e, norm %.3e; yardstick: 1 - cos %.3e / %.3e, norm %.3e / %.3e; bars %.3e, %.3e"
          % (cos, norm, yard[0][0], yard[1][0], yard[0][1], yard[1][1], bar_cos, bar_norm))
    assert cos <= bar_cos and norm <= bar_norm, (cos, norm, yard)


def _trainer(tmp_path, *opts):
    import logging
    from rnd_semantic_segmentation_amd.host import config as hc, pranet
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "SOLVER.EPOCHS", 1, "SOLVER.BASE_LR", 1e-4, "INPUT.TRAINSIZE", 160, "SOLVER.LOSS", "tversky"] + list(opts))
    cfg.freeze()
    log = logging.getLogger("pranet_sdf")
    log.addHandler(logging.NullHandler())
    torch.manual_seed(11)
    tr = pranet.PraNetTrainer("pranet", cfg, None, 0, logger=log)
    tr.model.train()
    return tr


def test_trainer_step_with_the_boundary_weight(K, tmp_path, monkeypatch):
    """A step with the key on runs, moves the parameters and gives the losses of PraNet.losses with that weight; with BOUNDARY_WEIGHT 0 the step's losses
    and parameters are bit-equal to the plain Tversky step, and neither mi_signed_distance nor the heads' phi mode is launched."""
    monkeypatch.setenv("MI_GRAPH", "0")
    x, gt = _pranet_inputs()
    tr = _trainer(tmp_path, "SOLVER.BOUNDARY_WEIGHT", 0.01)
    assert tr.boundary_weight == 0.01
    before = tr.model._store.data.clone()
    ls = [l.detach().clone() for l in tr.train_step(x, gt)]
    torch.cuda.synchronize()
    assert len(ls) == 4 and all(np.isfinite(float(l)) for l in ls) and not torch.equal(before, tr.model._store.data)
    want = _trainer(tmp_path, "SOLVER.BOUNDARY_WEIGHT", 0.01).model.losses(x, gt, boundary_weight=0.01)
    assert all(torch.equal(a, b.detach()) for a, b in zip(ls, want))

    plain = _trainer(tmp_path)
    plain_ls = [l.detach().clone() for l in plain.train_step(x, gt)]
    assert not any(torch.equal(a, b) for a, b in zip(ls, plain_ls))

    def refuse(*a, **k):
        raise AssertionError("launched with SOLVER.BOUNDARY_WEIGHT 0")
    real = K.upsample_tversky_bce
    monkeypatch.setattr(K, "signed_distance", refuse)
    monkeypatch.setattr(K, "upsample_tversky_bce", lambda *a, **k: refuse() if ("phi" in k or "w_boundary" in k) else real(*a, **k))
    off = _trainer(tmp_path, "SOLVER.BOUNDARY_WEIGHT", 0.0)
    off_ls = [l.detach().clone() for l in off.train_step(x, gt)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(off_ls, plain_ls)) and torch.equal(off.model._store.data, plain.model._store.data)


def test_graph_replay_is_bit_equal_to_eager(K, tmp_path, monkeypatch):
    """PraNetTrainer.train_step with SOLVER.BOUNDARY_WEIGHT 0.01, MI_GRAPH off against on (three eager steps, then the captured step replayed),
    2 x 3 x 96 x 96 on changing inputs - the distance map is computed inside the graph from the new mask: identical losses after every step and
    identical parameters after five."""
    data = [synth.synth_polyp(2, 96, 96, seed=60 + i) for i in range(5)]

    def run(graph):
        monkeypatch.setenv("MI_GRAPH", "1" if graph else "0")
        tr = _trainer(tmp_path, "SOLVER.BOUNDARY_WEIGHT", 0.01, "INPUT.TRAINSIZE", 96)
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
    assert len({tuple(step) for step in eager}) == 5
