"""CPU tests of the boundary (signed-distance) loss's host side: the exhaustive d2 / phi of tests/_sdf_ref.py against scipy's distance_transform_edt
through the published line edt(~G) * ~G - (edt(G) - 1) * G (bit for bit, in float64 and after the float32 cast), the written-out gradient of
losses.BoundaryLoss's Function, the SOLVER.BOUNDARY_WEIGHT key, the YAML, the refusals of the trainers, and the argument checks of
mi_signed_distance and mi_upsample_tversky_bce_sdf (which return before any launch: the library loads without a GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _sdf_ref as S
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import gald, gald_fada, losses, pranet, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "2x5x7": lambda: S.blobs("sdf.a", 2, 5, 7),
    "1x37x70": lambda: S.blobs("sdf.b", 1, 37, 70),
    "speckle": lambda: S.speckle("sdf.c", 2, 33, 45),
    "mixed": S.mixed_batch,
    "soft": S.soft_mask,
    "nan": S.nan_mask,
}


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_scipy_line_bit_for_bit(name):
    ndi = pytest.importorskip("scipy.ndimage")
    mask = CASES[name]()
    d2, G = S.d2_ref(mask)
    phi = S.phi_of(d2, G)
    assert d2.dtype == np.int32 and phi.dtype == np.float32 and np.array_equal(G, S.foreground(mask))
    for b in range(mask.shape[0]):
        g = G[b]
        if not g.any() or g.all():          # no contour: the published code returns zeros for an empty foreground; edt has nothing to measure to
            assert not d2[b].any() and not phi[b].any()
            continue
        line = ndi.distance_transform_edt(~g) * ~g - (ndi.distance_transform_edt(g) - 1) * g          # float64
        s = np.sqrt(d2[b].astype(np.float64))
        mine = np.where(g, 1.0 - s, s)          # 1 - s is -(s - 1) with +0 at s = 1, as the line gives it (0 * 0 - 0 * 1)
        assert np.array_equal(mine, line), (name, b)
        assert phi[b].tobytes() == line.astype(np.float32).tobytes(), (name, b)
        assert (phi[b][~g] >= 1.0).all() and (phi[b][g] <= 0.0).all()
    if name == "soft":
        assert G[0, 3:9, 10:30].all() and not G[0, 9:14, 10:30].any()          # exactly 0.5 is foreground, the float below it is not
    if name == "nan":
        assert not G[0, 5:9, 4:20].any() and not G[1, :, 30].any()


def test_written_out_boundary_gradient_is_the_autograd_gradient():
    torch.manual_seed(3)
    pred = torch.randn(2, 1, 9, 11, dtype=torch.float64, requires_grad=True)
    phi = torch.from_numpy(S.phi_ref(S.blobs("sdf.g", 2, 9, 11))).double().unsqueeze(1)
    loss = losses._BoundaryFn.apply(pred, phi)
    loss.backward(torch.tensor(1.7, dtype=torch.float64))
    ref = pred.detach().clone().requires_grad_(True)
    want = (torch.sigmoid(ref) * phi).mean()
    want.backward(torch.tensor(1.7, dtype=torch.float64))
    assert abs(float(loss.detach()) - float(want.detach())) < 1e-15 and (pred.grad - ref.grad).abs().max() < 1e-15
    r = S.sdf_loss_ref(pred.detach()[:, 0], torch.zeros(2, 9, 11), phi[:, 0], weights=(0.0, 0.0), w_boundary=1.0)
    assert abs(float(r.loss) - float(want.detach())) < 1e-15 and abs(float(r.boundary) - float(want.detach())) < 1e-15


def _cfg(*opts, yaml=None):
    c = hc.CfgNode(hc.default_tree())
    if yaml:
        c.merge_from_file(yaml)
    c.merge_from_list(list(opts))
    return c


def test_config_key_merges_and_refuses_other_values(tmp_path):
    assert _cfg().SOLVER.BOUNDARY_WEIGHT == 0.0
    assert _cfg("SOLVER.BOUNDARY_WEIGHT", "0.01").SOLVER.BOUNDARY_WEIGHT == 0.01
    assert _cfg("SOLVER.BOUNDARY_WEIGHT", 2).SOLVER.BOUNDARY_WEIGHT == 2.0
    for value in (-0.01, "-1", "much", "nan", True, [0.1]):
        with pytest.raises(ValueError, match="SOLVER.BOUNDARY_WEIGHT"):
            _cfg("SOLVER.BOUNDARY_WEIGHT", value)
    path = tmp_path / "bad.yaml"
    path.write_text("SOLVER:\n  BOUNDARY_WEIGHT: -0.5\n")
    with pytest.raises(ValueError, match="SOLVER.BOUNDARY_WEIGHT"):
        _cfg(yaml=str(path))


def test_the_yaml_loads():
    c = _cfg(yaml=os.path.join(ROOT, "configs", "pranet_src_kvasir_boundary.yaml"))
    assert c.SOLVER.LOSS == "tversky" and c.SOLVER.BOUNDARY_WEIGHT == 0.01 and c.SOLVER.TVERSKY_ALPHA == 0.7 and c.AUG.NAME == "pra"
    plain = _cfg(yaml=os.path.join(ROOT, "configs", "pranet_src_kvasir.yaml"))
    assert plain.SOLVER.LOSS == "ce" and plain.SOLVER.BOUNDARY_WEIGHT == 0.0
    for k in ("MODEL", "DATASETS", "INPUT", "TEST", "AUG"):
        assert c[k] == plain[k]


@pytest.mark.parametrize("make", [
    lambda c: trainer.ASPPTrainer("t", c, None, 0),
    lambda c: gald.GALDTrainer("t", c, None, 0),
    lambda c: gald_fada.GaldFada("t", c, None, None, 0),
], ids=["ASPPTrainer", "GALDTrainer", "GaldFada"])
def test_other_trainers_refuse_the_boundary_weight(tmp_path, make):
    with pytest.raises(NotImplementedError, match="PraNetTrainer"):
        make(_cfg("SOLVER.BOUNDARY_WEIGHT", 0.01, "OUTPUT_DIR", str(tmp_path)))


def test_the_adversarial_and_classmix_combos_refuse_the_boundary_weight(tmp_path):
    from rnd_semantic_segmentation_amd.host import fada, self_train
    c = _cfg("SOLVER.BOUNDARY_WEIGHT", 0.01, "OUTPUT_DIR", str(tmp_path))
    for combo in (fada.AsppFada, self_train.AsppClassMix):
        with pytest.raises(NotImplementedError, match="PraNetTrainer"):
            combo("t", c, None, None, 0)


def test_pranet_trainer_needs_the_tversky_loss_for_it(tmp_path):
    with pytest.raises(ValueError, match="SOLVER.BOUNDARY_WEIGHT.*SOLVER.LOSS"):
        pranet.PraNetTrainer("t", _cfg("SOLVER.BOUNDARY_WEIGHT", 0.01, "OUTPUT_DIR", str(tmp_path)), None, 0)
    assert pranet.PraNetTrainer.LOSSES == ("ce", "tversky")
    net = pranet.PraNet()
    x, gt = torch.zeros(1, 3, 32, 32), torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="boundary_weight"):
        net.losses(x, gt, boundary_weight=-1.0)
    with pytest.raises(ValueError, match="boundary_weight"):
        pranet.step_losses(net, x, gt, "tversky", boundary_weight=float("nan"))
    with pytest.raises(ValueError, match="boundary_weight"):
        pranet.step_losses(net, x, gt, "ce", boundary_weight=0.01)
    assert net.__dict__.get("_tversky") is None


def test_boundary_loss_refuses_cpu_tensors_and_several_channels():
    pred, lab = torch.zeros(2, 1, 4, 5), torch.zeros(2, 1, 4, 5)
    for crit in (losses.BoundaryLoss(), losses.CompoundLoss([losses.TverskyLoss(), losses.BoundaryLoss()], weights=[0.0, 1.0])):
        with pytest.raises(NotImplementedError, match="MI355X only"):
            crit(pred, lab)

    class Fake:
        is_cuda, device = True, "cuda:0"

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)
    with pytest.raises(NotImplementedError, match="C > 1"):
        losses.boundary(Fake(2, 3, 4, 5), Fake(2, 3, 4, 5))
    with pytest.raises(ValueError, match="does not match"):
        losses.boundary(Fake(2, 1, 4, 5), Fake(2, 1, 4, 6))


@pytest.fixture(scope="module")
def L():
    try:
        return _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)


def test_signed_distance_argument_checks_refuse_before_any_launch(L):
    one = ctypes.c_void_p(256)          # non-null dummy: every check below fails before anything is dereferenced or launched

    def call(mask=one, phi=one, ws=one, thresh=0.5, B=2, H=20, W=28, nbytes=1 << 30):
        return L.mi_signed_distance(mask, thresh, phi, None, None, B, H, W, ws, nbytes, None)

    for kw in (dict(mask=None), dict(phi=None), dict(ws=None)):
        assert call(**kw) == -22 and b"null operand" in L.mi_last_error(), kw
    assert call(B=0) == -22 and call(H=0) == -22 and call(W=-1) == -22 and b"bad dimension" in L.mi_last_error()
    assert call(H=4097) == -22 and call(W=4097) == -22 and call(B=65536) == -22 and b"beyond the limits" in L.mi_last_error()
    for t in (float("nan"), float("inf"), -float("inf")):
        assert call(thresh=t) == -22 and b"thresh" in L.mi_last_error()
    need = L.mi_signed_distance_workspace(2, 20, 28)
    assert need >= 2 * 20 * 28 * 4 + 2 * 4
    rc = call(nbytes=need - 1)
    assert rc != 0 and rc != -22 and b"workspace too small" in L.mi_last_error()
    assert L.mi_signed_distance_workspace(0, 20, 28) == 0 and L.mi_signed_distance_workspace(1, 4097, 8) == 0
    assert L.mi_signed_distance_workspace(1, 4096, 4096) >= 4096 * 4096 * 4


def test_sdf_head_argument_checks_refuse_before_any_launch(L):
    one = ctypes.c_void_p(256)

    def call(low=one, mask=one, phi=one, out=one, ws=one, B=2, h=5, w=7, H=20, W=28, alpha=0.7, eps=1.0, wbd=0.01, nbytes=1 << 30):
        return L.mi_upsample_tversky_bce_sdf(low, mask, phi, out, None, None, B, h, w, H, W, alpha, eps, 0.5, 0.5, wbd, 1.0, 0, ws, nbytes, None)

    for kw in (dict(low=None), dict(mask=None), dict(phi=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == -22 and b"null operand" in L.mi_last_error(), kw
    for wbd in (-0.01, float("nan"), float("inf")):
        assert call(wbd=wbd) == -22 and b"w_boundary" in L.mi_last_error()
    assert call(B=0) == -22 and b"bad dimension" in L.mi_last_error()
    assert call(H=4) == -22 and b"only upsampling" in L.mi_last_error()
    assert call(alpha=1.5) == -22 and b"alpha" in L.mi_last_error()
    assert call(eps=0.0) == -22 and b"eps" in L.mi_last_error()
    need, plain = L.mi_upsample_tversky_bce_sdf_workspace(2, 5, 7, 20, 28), L.mi_upsample_tversky_bce_workspace(2, 5, 7, 20, 28)
    assert need > plain          # one more partial per workgroup
    rc = call(nbytes=need - 1)
    assert rc != 0 and rc != -22 and b"workspace too small" in L.mi_last_error() and b"_sdf" in L.mi_last_error()
    assert L.mi_upsample_tversky_bce_sdf_workspace(0, 5, 7, 20, 28) == 0
