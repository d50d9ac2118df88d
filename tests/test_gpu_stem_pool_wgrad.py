"""The stem weight gradient that builds dy from the pooled gradient inside its launch (mi_stem_conv_wgrad_pool, csrc/stem_direct.hip) against the two
launches it replaces, mi_stem_pool_bwd + mi_stem_conv_wgrad: the same bits, bit for bit (torch.equal on integer views).

Shapes (B, H, W) of the image; the conv output is (Ho, Wo) = ((H - 1) // 2 + 1, ...), the pooled map (Hp, Wp) = ((Ho - 1) // 2 + 1, ...):
  (2, 33, 33)   conv 17 x 17 (odd), pooled 9 x 9: a partial row tile (17 = 4 * 4 + 1) whose last conv row has one window row only
  (1, 40, 72)   conv 20 x 36 (even), pooled 10 x 18: the last conv row / column lies in ONE window (no pooled row / column to the right of it)
  (2, 257, 131) conv 129 x 66, pooled 65 x 33: two column tiles, the second 2 columns wide (its pooled patch runs past Wp), 132 tiles, two images
The argmax bytes come from mi_stem_pool_fwd on a random conv output (ties between equal bf16 values, and 9 = "no gradient" where the pooled value is 0)
and, separately, uniformly from 0..9.  The BatchNorm scale has both signs (a negative scale turns an empty sum into -0).
The first shape is also held against a float64 conv2d weight gradient at the bound of tests/test_gpu_stem_direct.py (2e-5 of the maximum: fp32
accumulation of bf16 products against exact math).  Child processes repeat everything with MI_STEM_WGRAD_SPLITS = 3 and 70 (many tiles per workgroup:
the register-carried patch of the next tile, tile decoding across images; a partition that does not divide)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
DEV = "cuda"
SHAPES = [(2, 33, 33), (1, 40, 72), (2, 257, 131)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _kern():
    global K
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rnd_semantic_segmentation_amd import kernels
    K = kernels
    yield


def out_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


_CASES = {}


def case(B, H, W):
    """Operands of one shape on the CPU, made once and shared."""
    key = (B, H, W)
    if key not in _CASES:
        g = torch.Generator(device="cpu").manual_seed(H * 11 + W)
        Ho, Wo = out_hw(H, W)
        Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
        x = torch.randn(B, 3, H, W, generator=g)
        # a coarse grid of values: equal neighbours (ties) are common, and about half of the pooled values of a channel with a negative shift are 0
        y = (torch.randint(-3, 4, (B, Ho, Wo, 64), generator=g).float() * 0.5).to(torch.bfloat16)
        scale = (torch.rand(64, generator=g) + 0.5) * torch.where(torch.rand(64, generator=g) < 0.25, -1.0, 1.0)
        shift = torch.randn(64, generator=g) * 0.5
        dpool = torch.randn(B, Hp, Wp, 64, generator=g).to(torch.bfloat16)
        idx_rand = torch.randint(0, 10, (B, Hp, Wp, 64), generator=g).to(torch.uint8)
        _CASES[key] = dict(x=x, y=y, scale=scale, shift=shift, dpool=dpool, idx_rand=idx_rand, conv_hw=(Ho, Wo))
    return _CASES[key]


def _both(c, idx):
    x4 = K.stem_pack_image(c["x"].to(DEV))
    dpool, scale = c["dpool"].to(DEV), c["scale"].to(DEV)
    two = K.stem_wgrad_direct(K.stem_pool_bwd(dpool, idx, scale, c["conv_hw"]), x4)
    one = K.stem_wgrad_pool(dpool, idx, scale, x4)
    return one, two


def _check_shape(B, H, W):
    c = case(B, H, W)
    _, idx = K.stem_pool_fwd(c["y"].to(DEV), c["scale"].to(DEV), c["shift"].to(DEV))
    hist = torch.bincount(idx.flatten().long(), minlength=10)
    assert int(hist[9]) > 0 and int((hist[:9] > 0).sum()) == 9, hist          # every tap and the "no gradient" byte occur
    for name, ix in (("pool_fwd", idx), ("uniform", c["idx_rand"].to(DEV))):
        one, two = _both(c, ix)
        assert one.shape == (64, 3, 7, 7) and one.dtype == torch.float32
        assert bool(torch.isfinite(two).all()) and float(two.abs().max()) > 0
        assert torch.equal(one.view(torch.int32), two.view(torch.int32)), (B, H, W, name)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_entry_has_the_bits_of_pool_backward_plus_weight_gradient(B, H, W):
    _check_shape(B, H, W)


def test_against_float64_conv2d_weight_gradient():
    B, H, W = SHAPES[0]
    c = case(B, H, W)
    idx = c["idx_rand"].to(DEV)
    dy = K.stem_pool_bwd(c["dpool"].to(DEV), idx, c["scale"].to(DEV), c["conv_hw"])
    ref = torch.nn.grad.conv2d_weight(c["x"].to(torch.bfloat16).double(), (64, 3, 7, 7), dy.cpu().double().permute(0, 3, 1, 2), stride=2, padding=3).numpy()
    one, _ = _both(c, idx)
    err = np.abs(one.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max()
    print("fused stem weight gradient (%d,%d,%d) vs float64: relmax %.3e" % (B, H, W, err))
    assert err < 2e-5


_CHILD_SPLITS = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_stem_pool_wgrad as t
from rnd_semantic_segmentation_amd import _lib, kernels
t.K = kernels
splits = %d
for B, H, W in t.SHAPES:
    Ho, Wo = t.out_hw(H, W)
    tiles = B * ((Ho + 3) // 4) * ((Wo + 63) // 64)
    assert _lib.lib().mi_stem_conv_wgrad_workspace(B, Ho, Wo) == min(tiles, splits) * 64 * 7 * 32 * 4       # the switch is in force
    t._check_shape(B, H, W)
print("splits ok")
"""


@pytest.mark.parametrize("splits", [3, 70])
def test_many_tiles_per_workgroup(splits):
    env = dict(os.environ, MI_STEM_WGRAD_SPLITS=str(splits))
    r = subprocess.run([sys.executable, "-c", _CHILD_SPLITS % (ROOT, os.path.join(ROOT, "tests"), splits)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "splits ok" in r.stdout, r.stdout + r.stderr


def _stem_fn_dw(B, H, W):
    from rnd_semantic_segmentation_amd.host import engine
    c = case(B, H, W)
    w = (torch.randn(64, 3, 7, 7, generator=torch.Generator(device="cpu").manual_seed(3)) * 0.1).to(DEV).requires_grad_(True)
    pool = engine.StemFn.apply(c["x"].to(DEV), w, c["scale"].to(DEV), c["shift"].to(DEV))
    pool.backward(c["dpool"].to(DEV))
    return w.grad


_CHILD_OFF = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import test_gpu_stem_pool_wgrad as t
from rnd_semantic_segmentation_amd import kernels
t.K = kernels
assert not kernels.stem_pool_wgrad_enabled()
called = []
fused = kernels.stem_wgrad_pool
kernels.stem_wgrad_pool = lambda *a, **k: (called.append(1), fused(*a, **k))[1]
torch.save(t._stem_fn_dw(*t.SHAPES[0]).cpu(), %r)
assert not called
print("switch off ok")
"""


def test_stem_fn_gives_the_same_weight_gradient_with_the_switch_on_and_off(tmp_path, monkeypatch):
    """MI_STEM_POOL_WGRAD is read once per process, hence the child for 0.  Here (default) StemFn.backward takes the fused entry."""
    out = str(tmp_path / "dw_off.pt")
    env = dict(os.environ, MI_STEM_POOL_WGRAD="0")
    r = subprocess.run([sys.executable, "-c", _CHILD_OFF % (ROOT, os.path.join(ROOT, "tests"), out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "switch off ok" in r.stdout, r.stdout + r.stderr
    assert K.stem_pool_wgrad_enabled()
    called = []
    fused, unfused = K.stem_wgrad_pool, K.stem_pool_bwd
    monkeypatch.setattr(K, "stem_wgrad_pool", lambda *a, **k: (called.append("fused"), fused(*a, **k))[1])
    monkeypatch.setattr(K, "stem_pool_bwd", lambda *a, **k: (called.append("pool_bwd"), unfused(*a, **k))[1])
    dw_on = _stem_fn_dw(*SHAPES[0])
    assert called == ["fused"]
    assert torch.equal(dw_on.cpu().view(torch.int32), torch.load(out).view(torch.int32))
