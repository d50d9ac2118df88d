"""ce_finalize_kernel (csrc/upsample_ce.hip), the one-workgroup sum between pass 1 and pass 2 of every fused upsample + CE head: its loads are issued in
batches of 16 pairs, its additions keep their order - thread t adds partial pairs t, t + 256, ... in ascending order, then the fixed tree of block_sum2.
The test reads the partial (loss, count) pairs that pass 1 of mi_upsample_ce left in the workspace (the first B * H * tiles float pairs), restates that
order in numpy float32 and wants loss_out[0:2] bit for bit.

Partial counts: 200 (below the 256 threads), 256 (every thread one pair), 300 (44 threads two pairs), 4 200 (the batched loop runs for threads 0..103 and
not for the others, the tail loop for all) - with a 5-column logit map every image row is one tile, so the count is B * H."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _tiles(w, W):                      # pick_jt of csrc/upsample_common.h
    f = (W + w - 1) // w
    jt = 32
    while jt > 4 and jt * f > 256:
        jt >>= 1
    return (w + jt - 1) // jt


def _restate(pairs):
    n = pairs.shape[0]
    acc = np.zeros((256, 2), np.float32)
    for i in range(0, n, 256):
        m = min(256, n - i)
        acc[:m] = acc[:m] + pairs[i:i + m]              # thread t, ascending i: one float32 addition each
    w = 128
    while w > 0:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w >>= 1
    return acc[0, 0], acc[0, 1]


@pytest.mark.parametrize("B,H", [(1, 200), (2, 128), (3, 100), (8, 525)])
def test_loss_and_count_are_the_ordered_sum_of_the_partial_pairs(B, H):
    from rnd_semantic_segmentation_amd import kernels as K
    h, w, W, C = 7, 5, 33, 19
    assert _tiles(w, W) == 1
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + H)
    low = torch.randn(B, h, w, C, generator=g).cuda()
    lab = torch.randint(0, C, (B, H, W), generator=g)
    lab[torch.rand(B, H, W, generator=g) < 0.1] = 255
    out, _ = K.upsample_ce(low, lab.cuda(), want_grad=False)
    n = B * H * _tiles(w, W)
    ws = K._workspace(0, low.device, "upce")
    pairs = ws[:n * 8].view(torch.float32).view(n, 2).cpu().numpy()
    got = out.cpu().numpy()
    s, c = _restate(pairs)
    assert c > 0 and float(pairs[:, 1].sum()) == float((lab != 255).sum())          # these are the pairs of this call: the counts are exact integers
    assert got[1].view(np.int32) == np.float32(c).view(np.int32)
    assert got[0].view(np.int32) == np.float32(s / c).view(np.int32)
