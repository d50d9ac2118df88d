"""GPU parity of the stem conv on raw image rows (csrc/stem_direct.hip): image pack, forward and weight gradient against float64 torch references on
the same bf16-rounded operands.

Bounds are those the suite already applies to this conv (test_gpu_ops.py, patch-matrix route): relmax < 2**-8 for y (a bf16 output: one ulp of the
largest magnitude) and < 2e-5 for dW (fp32 accumulation of bf16 products against exact math).
The forward contracts in the order of the patch-matrix GEMM it replaces, so y must also have exactly that route's bits.

Shapes: odd sizes and two images (2,33,35); (1,65,65); B = 3 with an even H (3,16,23); an image smaller than one window row block, every tap partly
in the padding (1,7,9); several column tiles and few rows (1,12,300); Wo < 16, a single partial MFMA group (2,40,8); Wo = 65, one more than the 64-column
tile of both kernels (1,9,129).  Ho of 17 and 33 leave a partial row tile in the forward (8 rows) and in the weight gradient (4 rows).

The weight gradient splits its tiles of 4 x 64 output pixels over min(tiles, MI_STEM_WGRAD_SPLITS = 512) workgroups, and the shapes above have at most
10 tiles: one per workgroup.  WGRAD_SHAPES adds what the training shape runs (5 432 tiles over 512 workgroups): (2,257,131) has 132 tiles, so the
reducer takes its 64-wide unrolled branch twice and its scalar tail; (4,513,513) has 1 300 tiles over 512 workgroups, 2 or 3 per workgroup (an uneven
partition), so the persistent loop - next tile prefetched in registers, two-barrier LDS hand-over, tile decoding across image boundaries inside one
workgroup - runs.  A child process repeats the shapes with 3 splits (every workgroup walks many tiles of several images) and with 70 (a partition of
132 and 1 300 tiles that does not divide, reducer: one unrolled pass + 6)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
DEV = "cuda"
SHAPES = [(2, 33, 35), (1, 65, 65), (3, 16, 23), (1, 7, 9), (1, 12, 300), (2, 40, 8), (1, 9, 129)]
WGRAD_SHAPES = SHAPES + [(2, 257, 131), (4, 513, 513)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _kern():
    global K
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rnd_semantic_segmentation_amd import kernels
    K = kernels
    yield


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def out_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


_CASES = {}


def case(B, H, W):
    """Operands (CPU) and float64 references of one shape, computed once and shared by the tests."""
    key = (B, H, W)
    if key not in _CASES:
        g = torch.Generator(device="cpu").manual_seed(H * 7 + W)
        x = torch.randn(B, 3, H, W, generator=g)
        Ho, Wo = out_hw(H, W)
        dy = torch.randn(B, Ho, Wo, 64, generator=g).to(torch.bfloat16)
        w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
        xb = x.to(torch.bfloat16)
        y_ref = torch.nn.functional.conv2d(xb.double(), w.to(torch.bfloat16).double(), None, 2, 3).permute(0, 2, 3, 1)
        dw_ref = torch.nn.grad.conv2d_weight(xb.double(), (64, 3, 7, 7), dy.double().permute(0, 3, 1, 2), stride=2, padding=3)
        _CASES[key] = dict(x=x, xb=xb, dy=dy, w=w, y_ref=y_ref.numpy(), dw_ref=dw_ref.numpy())
    return _CASES[key]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_pack_image_is_the_bf16_cast_with_a_zero_fourth_channel(B, H, W):
    c = case(B, H, W)
    want = c["xb"].permute(0, 2, 3, 1)
    x4 = K.stem_pack_image(c["x"].to(DEV))                                                       # fp32 NCHW
    assert x4.shape == (B, H, W, 4) and x4.dtype == torch.bfloat16
    assert torch.equal(x4[..., :3].cpu().view(torch.int16), want.contiguous().view(torch.int16))
    assert bool((x4[..., 3].view(torch.int16) == 0).all())
    x4b = K.stem_pack_image(c["xb"].to(DEV).contiguous(memory_format=torch.channels_last))       # bf16 channels_last
    assert torch.equal(x4b.view(torch.int16), x4.view(torch.int16))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_forward_vs_float64_conv2d(B, H, W):
    c = case(B, H, W)
    x4 = K.stem_pack_image(c["x"].to(DEV))
    wd = c["w"].to(DEV)
    y = K.stem_conv_direct(x4, wd)
    err = relmax(y.float().cpu().numpy(), c["y_ref"])
    print("forward (%d,%d,%d): relmax %.3e" % (B, H, W, err))
    assert y.shape == c["y_ref"].shape
    assert err < 2.0 ** -8
    assert torch.equal(y.view(torch.int16), K.stem_conv_direct(x4, wd).view(torch.int16))
    # the contraction runs in the order of the patch-matrix GEMM (same K = 32 steps, same element positions): the same bits as that route
    y_old, _ = K.stem_conv_fwd(c["xb"].to(DEV).contiguous(memory_format=torch.channels_last), wd)
    assert torch.equal(y.view(torch.int16), y_old.view(torch.int16))


def _check_weight_gradient(B, H, W):
    c = case(B, H, W)
    x4 = K.stem_pack_image(c["x"].to(DEV))
    dyd = c["dy"].to(DEV)
    dw = K.stem_wgrad_direct(dyd, x4)
    err = relmax(dw.cpu().numpy(), c["dw_ref"])
    print("weight gradient (%d,%d,%d): relmax %.3e" % (B, H, W, err))
    assert dw.shape == (64, 3, 7, 7) and dw.dtype == torch.float32
    assert err < 2e-5
    assert torch.equal(dw.view(torch.int32), K.stem_wgrad_direct(dyd, x4).view(torch.int32))


@pytest.mark.parametrize("B,H,W", WGRAD_SHAPES)
def test_weight_gradient_vs_float64_conv2d_weight(B, H, W):
    _check_weight_gradient(B, H, W)


_CHILD_SPLITS = """
import ctypes, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_stem_direct as t
from rnd_semantic_segmentation_amd import _lib, kernels
t.K = kernels
splits = %d
for B, H, W in t.WGRAD_SHAPES:
    Ho, Wo = t.out_hw(H, W)
    tiles = B * ((Ho + 3) // 4) * ((Wo + 63) // 64)
    assert _lib.lib().mi_stem_conv_wgrad_workspace(B, Ho, Wo) == min(tiles, splits) * 64 * 7 * 32 * 4       # the switch is in force
    t._check_weight_gradient(B, H, W)
print("splits ok")
"""


@pytest.mark.parametrize("splits", [3, 70])
def test_weight_gradient_with_many_tiles_per_workgroup(splits):
    """MI_STEM_WGRAD_SPLITS (read once per process, hence the child): the same bounds and the same run-to-run bit-equality on every shape when a
    workgroup walks many tiles (3: up to 434 each, across image boundaries) and when the tiles do not divide over the workgroups (70)."""
    env = dict(os.environ, MI_STEM_WGRAD_SPLITS=str(splits))
    r = subprocess.run([sys.executable, "-c", _CHILD_SPLITS % (ROOT, os.path.join(ROOT, "tests"), splits)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "splits ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("B,H,W,where", [(2, 33, 35, "interior"), (2, 33, 35, "last_column"), (1, 12, 300, "interior"), (1, 12, 300, "last_column"),
                                         (1, 9, 129, "last_column")])
def test_one_nan_pixel_poisons_exactly_what_it_poisons_in_torch(B, H, W, where):
    """A NaN pixel makes non-finite exactly the outputs whose window holds it and exactly the weight-gradient taps that meet it: the elements k = 28..31
    of a window (the pixel right of it) and the pixels past Wo of a tile are multiplied by zeros in the kernels, and 0 * NaN would spread it."""
    c = case(B, H, W)
    x = c["x"].clone()
    h, w_ = H // 2, (W // 2 if where == "interior" else W - 1)
    x[B - 1, :, h, w_] = float("nan")
    xb = x.to(torch.bfloat16)
    y_ref = torch.nn.functional.conv2d(xb.double(), c["w"].to(torch.bfloat16).double(), None, 2, 3).permute(0, 2, 3, 1)
    dw_ref = torch.nn.grad.conv2d_weight(xb.double(), (64, 3, 7, 7), c["dy"].double().permute(0, 3, 1, 2), stride=2, padding=3)
    x4 = K.stem_pack_image(x.to(DEV))
    y = K.stem_conv_direct(x4, c["w"].to(DEV)).float().cpu()
    dw = K.stem_wgrad_direct(c["dy"].to(DEV), x4).cpu()
    assert 0 < int((~torch.isfinite(y_ref)).sum()) < y_ref.numel()
    assert torch.equal(torch.isfinite(y), torch.isfinite(y_ref))
    assert torch.equal(torch.isfinite(dw), torch.isfinite(dw_ref))
    ok = torch.isfinite(y_ref)
    assert relmax(y[ok].numpy(), y_ref[ok].numpy()) < 2.0 ** -8
    okw = torch.isfinite(dw_ref)
    if bool(okw.any()):
        assert relmax(dw[okw].numpy(), dw_ref[okw].numpy()) < 2e-5


def _stem_fn_bits(B, H, W):
    """StemFn forward and backward through the engine, and the same through the patch-matrix kernels called one by one."""
    from rnd_semantic_segmentation_amd.host import engine
    c = case(B, H, W)
    g = torch.Generator(device="cpu").manual_seed(5)
    scale = (torch.rand(64, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(64, generator=g) * 0.1).to(DEV)
    wd = c["w"].to(DEV).requires_grad_(True)
    pool = engine.StemFn.apply(c["x"].to(DEV), wd, scale, shift)
    dpool = torch.randn(pool.shape, generator=g).to(torch.bfloat16).to(DEV)
    pool.backward(dpool)
    xcl = c["xb"].to(DEV).contiguous(memory_format=torch.channels_last)
    y, col = K.stem_conv_fwd(xcl, wd.detach())
    pool_old, idx = K.stem_pool_fwd(y, scale, shift)
    dw_old = K.stem_wgrad(K.stem_pool_bwd(dpool, idx, scale, (y.shape[1], y.shape[2])), col=col)
    return pool.detach(), wd.grad, pool_old, dw_old


_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import test_gpu_stem_direct as t
from rnd_semantic_segmentation_amd import kernels
t.K = kernels
assert not kernels.stem_direct_enabled()
pool, dw, pool_old, dw_old = t._stem_fn_bits(2, 33, 35)
assert torch.equal(pool.view(torch.int16), pool_old.view(torch.int16))
assert torch.equal(dw.view(torch.int32), dw_old.view(torch.int32))
print("old route bits ok")
"""


def test_switch_off_restores_the_patch_matrix_route_bit_for_bit():
    """MI_STEM_DIRECT=0 (read once per process, hence the child): StemFn gives the bits of mi_stem_im2col + GEMM and of the 1x1 weight gradient on the
    patch matrix.  In this process (default) StemFn gives the bits of the direct kernels called one by one."""
    env = dict(os.environ, MI_STEM_DIRECT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "old route bits ok" in r.stdout, r.stdout + r.stderr
    assert K.stem_direct_enabled()
    pool, dw, _, _ = _stem_fn_bits(2, 33, 35)
    c = case(2, 33, 35)
    g = torch.Generator(device="cpu").manual_seed(5)
    scale = (torch.rand(64, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(64, generator=g) * 0.1).to(DEV)
    x4 = K.stem_pack_image(c["x"].to(DEV))
    y = K.stem_conv_direct(x4, c["w"].to(DEV))
    pool_new, idx = K.stem_pool_fwd(y, scale, shift)
    dpool = torch.randn(pool_new.shape, generator=g).to(torch.bfloat16).to(DEV)
    dw_new = K.stem_wgrad_direct(K.stem_pool_bwd(dpool, idx, scale, (y.shape[1], y.shape[2])), x4)
    assert torch.equal(pool.view(torch.int16), pool_new.view(torch.int16))
    assert torch.equal(dw.view(torch.int32), dw_new.view(torch.int32))
