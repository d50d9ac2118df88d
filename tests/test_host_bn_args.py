"""Argument validation of csrc/batchnorm.hip and csrc/colsum.hip without a GPU: every call below returns MI_EINVAL / MI_ENOMEM with a message before any launch
(the pointers are dummies that are never dereferenced; a launch on this machine would fail differently)."""
import ctypes

import pytest

import _bn_ref as R
from rnd_semantic_segmentation_amd import _lib

EINVAL, ENOMEM = -22, -12
ONE = 64          # a non-null, 16-byte aligned dummy address: validation fails before it is dereferenced


@pytest.fixture(scope="module")
def L():
    try:
        return _lib.lib()
    except _lib.MiError as e:
        pytest.fail("libmi355seg.so not built: %s" % e)


def _v(a):
    return None if a is None else ctypes.c_void_p(a)


def _reductions(L):
    """name -> call(M, C, ws_bytes) of the three reduction entries with valid dummy operands."""
    return {
        "mi_bn_colsum": lambda M, C, ws: L.mi_bn_colsum(_v(ONE), None, M, C, _v(ONE), _v(ONE), ws, None),
        "mi_bn_colsum2": lambda M, C, ws: L.mi_bn_colsum2(_v(ONE), _v(ONE), M, C, _v(ONE), _v(ONE), _v(ONE), ws, None),
        "mi_bn_bwd_colsums": lambda M, C, ws: L.mi_bn_bwd_colsums(_v(ONE), _v(ONE), _v(ONE), _v(ONE), None, M, C, _v(ONE), _v(ONE), _v(ONE), ws, None),
    }


def test_reductions_refuse_channel_counts_and_a_short_workspace_before_any_launch(L):
    for name, call in _reductions(L).items():
        for C in (12, 2056, 0):            # no multiple of 8; more than the 256 slots of a workgroup
            assert call(100, C, 1 << 30) == EINVAL and b"C a multiple of 8, at most 2048" in L.mi_last_error(), (name, C)
        assert call(0, 64, 1 << 30) == EINVAL and name.encode() in L.mi_last_error()
        need = L.mi_bn_workspace(100, 64)
        assert need == 256 * 2 * 64 * 4
        assert call(100, 64, need - 1) == EINVAL and b"workspace too small" in L.mi_last_error(), name      # one byte short


def test_apply_kernels_refuse_bad_channels_alignment_and_sign_bits_before_any_launch(L):
    def apply(mean=ONE, scale=ONE, beta=ONE, res=None, mask=None, M=10, C=64):
        return L.mi_bn_apply(_v(ONE), _v(mean), _v(scale), _v(beta), _v(res), _v(ONE), _v(mask), 1, M, C, None)

    def bwd(mean=ONE, invstd=ONE, gamma=ONE, dbeta=ONE, dgamma=ONE, bits=None, M=10, C=64):
        return L.mi_bn_bwd_apply(_v(ONE), _v(ONE), _v(mean), _v(invstd), _v(gamma), _v(dbeta), _v(dgamma), 0.1, _v(bits), _v(ONE), M, C, None)

    assert apply(C=12) == EINVAL and b"C a multiple of 8" in L.mi_last_error()
    assert bwd(C=12) == EINVAL and b"C a multiple of 8" in L.mi_last_error()
    # the kernels read 8 channels of each per-channel vector as two 16-byte loads: a vector at a 4-byte offset is refused
    for k in ("mean", "scale", "beta"):
        assert apply(**{k: ONE + 4}) == EINVAL and b"16-byte aligned" in L.mi_last_error(), k
    for k in ("mean", "invstd", "gamma", "dbeta", "dgamma"):
        assert bwd(**{k: ONE + 4}) == EINVAL and b"16-byte aligned" in L.mi_last_error(), k
    assert apply(res=ONE + 8) == EINVAL and b"residual alignment" in L.mi_last_error()
    # packed sign bits are one uint16 per 16 channels
    assert apply(mask=ONE, C=24) == EINVAL and b"sign bits need C % 16 == 0" in L.mi_last_error()
    assert bwd(bits=ONE, C=24) == EINVAL and b"16 with sign bits" in L.mi_last_error()
    assert apply(M=0) == EINVAL and bwd(M=0) == EINVAL


def test_finalize_refuses_an_empty_count_and_half_a_pair_of_running_buffers(L):
    def fin(count=10.0, rm=None, rv=None, gamma=ONE, C=64):
        return L.mi_bn_finalize(_v(ONE), _v(ONE), _v(ONE), count, _v(gamma), _v(ONE), _v(rm), _v(rv), None, 0.1, 1e-5, _v(ONE), C, None)

    assert fin(count=0.0) == EINVAL and b"count=0" in L.mi_last_error()
    assert fin(count=0.5) == EINVAL
    assert fin(rm=ONE) == EINVAL and b"mi_bn_finalize" in L.mi_last_error()           # running_mean without running_var
    assert fin(rv=ONE) == EINVAL
    assert fin(gamma=None) == EINVAL and fin(C=0) == EINVAL


def test_column_sums_refuse_wide_inputs_and_a_short_workspace_before_any_launch(L):
    aspp = lambda M=100, K=19, ws=1 << 30: L.mi_aspp_bias_grad(_v(ONE), _v(ONE), M, K, 0, _v(ONE), ws, None)
    bias = lambda M=100, N=64, ws=1 << 30, dy=ONE: L.mi_bias_grad_bf16(_v(dy), _v(ONE), M, N, 0, _v(ONE), ws, None)
    assert aspp(K=257) == EINVAL and b"too wide (at most 256 columns)" in L.mi_last_error()            # 257 slots round to 512 > 256 threads
    assert bias(N=2056) == EINVAL and b"too wide (at most 2048 columns)" in L.mi_last_error()
    assert bias(N=12) == EINVAL and b"N % 8 == 0" in L.mi_last_error()
    assert bias(dy=ONE + 8) == EINVAL
    assert aspp(M=0) == EINVAL and aspp(K=0) == EINVAL and bias(M=0) == EINVAL
    # the launch needs nblocks * N floats (tests/_bn_ref.py colsum_plan): one byte less is MI_ENOMEM
    for M, K in ((100, 19), (1, 1), (4097, 256)):
        need = R.colsum_plan(M, K, 1).nblocks * K * 4
        assert aspp(M=M, K=K, ws=need - 1) == ENOMEM and b"workspace too small" in L.mi_last_error(), (M, K)
    for M, N in ((100, 64), (4097, 2048)):
        need = R.colsum_plan(M, N, 8).nblocks * N * 4
        assert bias(M=M, N=N, ws=need - 1) == ENOMEM and b"workspace too small" in L.mi_last_error(), (M, N)
    assert L.mi_colsum_workspace(4097, 2048) == 512 * 2048 * 4
