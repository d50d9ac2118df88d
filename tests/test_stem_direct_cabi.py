"""CPU-side checks of the direct stem conv's C-ABI entry points (csrc/stem_direct.hip): every documented refusal fires before any launch, so none of
these calls needs a GPU (the pointers are never dereferenced)."""
import ctypes

import pytest

import __graft_entry__ as entry
from rnd_semantic_segmentation_amd import _lib


@pytest.fixture(scope="module")
def built():
    entry.build()
    return _lib.lib()


ONE = ctypes.c_void_p(16)          # non-null, 16-byte aligned dummy
ODD = ctypes.c_void_p(20)          # 4-byte aligned only


def test_pack_image_refusals(built):
    assert built.mi_stem_pack_image(None, 0, ONE, 1, 8, 8, None) == -22 and b"bad argument" in built.mi_last_error()
    assert built.mi_stem_pack_image(ONE, 0, ONE, 1, 0, 8, None) == -22 and b"bad argument" in built.mi_last_error()
    assert built.mi_stem_pack_image(ONE, 2, ONE, 1, 8, 8, None) == -22 and b"x_is_bf16_nhwc" in built.mi_last_error()
    assert built.mi_stem_pack_image(ONE, 0, ODD, 1, 8, 8, None) == -22 and b"alignment" in built.mi_last_error()
    assert built.mi_stem_pack_image(ONE, 0, ONE, 8, 16384, 16384, None) == -22 and b"32-bit" in built.mi_last_error()


def test_forward_refusals(built):
    def fwd(x4=ONE, w=ONE, wp=ONE, y=ONE, B=1, H=9, W=9, O=64, Ho=5, Wo=5):
        return built.mi_stem_conv_fwd(x4, w, wp, y, B, H, W, O, Ho, Wo, None)

    assert fwd(w=None) == -22 and b"null operand" in built.mi_last_error()
    assert fwd(O=32) == -22 and b"64 output channels" in built.mi_last_error()
    assert fwd(Ho=4) == -22 and b"7x7/2/3" in built.mi_last_error()
    assert fwd(Wo=6) == -22 and b"7x7/2/3" in built.mi_last_error()
    assert fwd(B=0) == -22 and b"positive" in built.mi_last_error()
    assert fwd(y=ODD) == -22 and b"alignment" in built.mi_last_error()
    assert fwd(x4=ODD) == -22 and b"alignment" in built.mi_last_error()
    assert fwd(B=64, H=4097, W=4097, Ho=2049, Wo=2049) == -22 and b"32-bit" in built.mi_last_error()


def test_weight_gradient_refusals(built):
    def wgrad(dy=ONE, x4=ONE, dw=ONE, B=1, H=9, W=9, O=64, Ho=5, Wo=5, ws=ONE, ws_bytes=1 << 30):
        return built.mi_stem_conv_wgrad(dy, x4, dw, B, H, W, O, Ho, Wo, ws, ws_bytes, None)

    need = built.mi_stem_conv_wgrad_workspace(1, 5, 5)
    assert need == 2 * 64 * 7 * 32 * 4                               # two tiles of 4 output rows: one partial [64][7][32] fp32 each
    import os
    if "MI_STEM_WGRAD_SPLITS" not in os.environ:
        assert built.mi_stem_conv_wgrad_workspace(8, 385, 385) == 512 * 64 * 7 * 32 * 4      # 5432 tiles over 512 workgroups
    assert built.mi_stem_conv_wgrad_workspace(0, 5, 5) == 0
    assert wgrad(ws=None) == -22 and b"null operand" in built.mi_last_error()
    assert wgrad(O=128) == -22 and b"64 output channels" in built.mi_last_error()
    assert wgrad(Ho=6) == -22 and b"7x7/2/3" in built.mi_last_error()
    assert wgrad(dy=ODD) == -22 and b"alignment" in built.mi_last_error()
    assert wgrad(ws_bytes=need - 1) == -22 and b"workspace holds" in built.mi_last_error()
    assert wgrad(B=64, H=4097, W=4097, Ho=2049, Wo=2049) == -22 and b"32-bit" in built.mi_last_error()


def test_switch_defaults_to_the_direct_route(built):
    import os
    if "MI_STEM_DIRECT" not in os.environ:
        assert built.mi_stem_direct_enabled() == 1
