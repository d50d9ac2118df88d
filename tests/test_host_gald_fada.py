"""CPU tests of GaldFada's host side (reference core/combos/gald_fada.py): the hardnet discriminator, configs/gald_adv.yaml, the argument
checks of the two-grid soft-label cross-entropy (mi_upsample_softce_2grid) and the entry points."""
import ctypes
import os

import pytest
import torch

from oracle import ref_model
from rnd_semantic_segmentation_amd import _lib
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import fada

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gald_adv_cfg():
    c = hc.CfgNode(hc.default_tree())
    c.merge_from_file(os.path.join(ROOT, "configs", "gald_adv.yaml"))
    return c


def test_hardnet_discriminator_matches_the_reference_layout():
    D = fada.build_adversarial_discriminator(gald_adv_cfg())
    ref = ref_model.RefPixelDiscriminator(1024, 256, 19)
    assert isinstance(D, fada.PixelDiscriminator)
    assert list(D.state_dict().keys()) == list(ref.state_dict().keys())
    assert {k: tuple(v.shape) for k, v in D.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert tuple(D.state_dict()["D.0.weight"].shape) == (256, 1024, 3, 3)
    D.load_state_dict(ref.state_dict())
    with pytest.raises(RuntimeError, match="MI355X only"):
        D.soft_loss_grids(torch.zeros(1, 1024, 2, 2), torch.zeros(1, 19, 8, 8), 0, (64, 64))
    c = gald_adv_cfg()
    c.merge_from_list(["MODEL.NAME", "gald_efficientnet"])
    with pytest.raises(NotImplementedError, match="hardnet"):
        fada.build_adversarial_discriminator(c)


def test_gald_adv_config_values():
    c = gald_adv_cfg()
    assert c.MODEL.NAME == "gald_hardnet" and c.MODEL.NUM_CLASSES == 19
    assert c.SOLVER.BATCH_SIZE == 5 and c.SOLVER.BATCH_SIZE // 2 == 2
    assert c.SOLVER.BASE_LR == 0.5e-4 and c.SOLVER.BASE_LR_D == 1e-4 and c.SOLVER.CHECKPOINT_PERIOD == 1 and c.SOLVER.EPOCHS == 10
    assert c.SOLVER.LR_METHOD == "poly" and c.SOLVER.LR_POWER == 0.9
    assert tuple(c.INPUT.SOURCE_INPUT_SIZE_TRAIN) == (1280, 720) and tuple(c.INPUT.TARGET_INPUT_SIZE_TRAIN) == (1024, 512)
    assert c.INPUT.IGNORE_LABEL == 255
    # the grids of the gald_adv geometry: linear2 at 1/4 resolution (stem conv 3x3/2 pad 1, max pool 3x3/2 pad 1: ceil halvings), HarDNet's last
    # feature after three more 2x2/2 max pools (floor halvings): 33-34x per axis to the full resolution
    for (w, h), seg, dgrid in (((1280, 720), (180, 320), (22, 40)), ((1024, 512), (128, 256), (16, 32))):
        q = lambda n: -(-(-(-n // 2)) // 2)
        assert (q(h), q(w)) == seg and (q(h) // 8, q(w) // 8) == dgrid


@pytest.fixture(scope="module")
def L():
    try:
        return _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)


def _call(L, seg=16, dl=16, out=16, ws=16, hs=8, wsz=8, sac=0, hd=2, wd=2, ldD=64, dac=1, domain=0, B=1, K=19, H=64, W=64, nbytes=1 << 30):
    v = lambda a: None if a is None else ctypes.c_void_p(a)
    return L.mi_upsample_softce_2grid(v(seg), hs, wsz, sac, 1 / 1.8, 0.9, v(dl), hd, wd, ldD, dac, domain, 1.0, v(out), None, B, K, H, W, v(ws),
                                      nbytes, None)


def test_softce_2grid_refuses_bad_arguments_before_any_launch(L):
    assert _call(L, seg=None) == -22 and b"null operand" in L.mi_last_error()
    assert _call(L, dl=None) == -22 and b"null operand" in L.mi_last_error()
    assert _call(L, out=None) == -22 and b"null operand" in L.mi_last_error()
    assert _call(L, ws=None) == -22 and b"null operand" in L.mi_last_error()
    assert _call(L, domain=2) == -22 and b"domain" in L.mi_last_error()
    assert _call(L, domain=-1) == -22 and b"domain" in L.mi_last_error()
    assert _call(L, K=33) == -22 and b"K = 33" in L.mi_last_error()
    assert _call(L, K=0) == -22 and b"K = 0" in L.mi_last_error()
    assert _call(L, K=19, ldD=37) == -22 and b"ldD = 37 < 2K = 38" in L.mi_last_error()
    assert _call(L, K=32, ldD=63) == -22 and b"ldD" in L.mi_last_error()
    assert _call(L, sac=2) == -22 and b"align_corners" in L.mi_last_error()
    assert _call(L, hd=65, H=64) == -22 and b"bad dimension" in L.mi_last_error()
    assert _call(L, wsz=0) == -22 and b"bad dimension" in L.mi_last_error()
    assert _call(L, H=70000, W=64) == -22 and b"overflow" in L.mi_last_error()
    assert _call(L, nbytes=16) == -12 and b"workspace too small" in L.mi_last_error()


def test_softce_2grid_workspace_query(L):
    # partial sums [B][H][wd] (256-byte aligned) + the x-gathered gradient rows [B][H][wd][2K]
    B, hd, wd, K, H, W = 2, 22, 40, 19, 720, 1280
    n = L.mi_upsample_softce_2grid_workspace(B, hd, wd, K, H, W)
    assert n >= B * H * wd * 2 * K * 4 + B * H * wd * 4
    assert n <= B * H * wd * 2 * K * 4 + B * H * wd * 4 + 256
    assert n < 10 << 20                                             # ~9 MB at the source geometry, nothing [B,C,H,W]-sized
    assert L.mi_upsample_softce_2grid_workspace(B, hd, wd, 32, H, W) > n
    assert L.mi_upsample_softce_2grid_workspace(1, 1, 1, 1, 1, 1) > 0


def test_entry_points():
    """train_adv.py --model gald_fada reaches the combo (a bad name is refused with the list); the combo is NOT served as
    core.combos.gald_fada (tests/test_host_fada.py pins that import as refused)."""
    from rnd_semantic_segmentation_amd.host import gald_fada
    assert gald_fada.GaldFada.trainer_cls.__name__ == "GALDTrainer" and gald_fada.GaldFada.adapter_cls is fada.FADAAdapter
    assert gald_fada.GaldFada.FUSED is True and gald_fada.GaldFada.TEMPERATURE == 1.8
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_adv_mod", os.path.join(ROOT, "train_adv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(NotImplementedError, match="gald_fada"):
        mod.main("attn_fada", gald_adv_cfg(), 0)
    with pytest.raises(ImportError, match="hot path"):
        import core.combos.gald_fada  # noqa: F401
