"""References, launch plans and DERIVED error bars for csrc/batchnorm.hip and csrc/colsum.hip (plain numpy / torch on the CPU, float64; no GPU).

Every bar here is an expression of the length of the kernel's fixed summation chain (`depth`), the unit roundoffs 2^-24 (fp32) and 2^-8 (one bf16
rounding, as the issue states it) and the operands' magnitudes.  None was obtained by running a kernel.

The bound on a sum.  A fixed-order fp32 sum in which one term passes through at most `depth` additions, each term itself carrying k fp32 roundings,
differs from the exact sum by at most (depth + k) * 2^-24 * A to first order, A = sum of the terms' magnitudes (Higham, Accuracy and Stability of
Numerical Algorithms, section 4.2: the bound depends on the depth of the summation tree only).  The second-order terms get one factor of 2 and
nothing else: bar[c] = 2 * (depth + k) * 2^-24 * A[c], per channel."""
import collections

import numpy as np
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
UBF = 2.0 ** -8           # one bf16 rounding of a result (8 significand bits)
Plan = collections.namedtuple("Plan", "slots cp L rows_per_block nblocks")


def cdiv(a, b):
    return -(-a // b)


def _pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def plan(M, C):
    """bn_plan of csrc/batchnorm.hip (lines 285-296): a thread owns 8 channels (slots = C / 8), the slots are rounded to a power of two cp, L = 256 / cp
    row lanes; M is cut into at most BN_MAX_BLOCKS = 256 blocks of rows_per_block rows, a multiple of L and at least L."""
    slots = C // 8
    cp = _pow2_at_least(slots)
    L = 256 // cp
    rpb = cdiv(M, 256)
    rpb = max(cdiv(rpb, L) * L, L)
    return Plan(slots, cp, L, rpb, cdiv(M, rpb))


def colsum_plan(M, N, vec):
    """launch() of csrc/colsum.hip (lines 69-76): slots = N / vec (vec 1: fp32 columns, 8: bf16x8 groups), cp <= 256, L = 256 / cp; at most
    MAX_BLOCKS = 512 blocks of rows = max(ceil(M / 512), 8 * L) rows - NOT rounded to a multiple of L."""
    slots = N // vec
    cp = _pow2_at_least(slots)
    assert cp <= 256, "colsum.hip refuses more than 256 slots"
    L = 256 // cp
    rows = max(cdiv(M, 512), 8 * L)
    return Plan(slots, cp, L, rows, cdiv(M, rows))


def depth(p):
    """Longest chain of fp32 additions one output of (bn_partial_kernel | colsum_partial_kernel) + (bn_final_kernel | colsum_final_kernel) goes through:
      ceil(rows_per_block / L)   a lane adds its rows r0 + rl, r0 + rl + L, ... in row order   (batchnorm.hip 71-90: the four-row trip keeps the order;
                                                                                                colsum.hip 25-33)
      + L                        lane 0 adds the L lane sums in LDS, ascending                   (batchnorm.hip 102-103; colsum.hip 41-42)
      + ceil(nblocks / 32)       lane q of the final kernel adds partials q, q + 32, ...         (batchnorm.hip 121; colsum.hip 57)
      + 32                       its lane 0 adds the 32 lane sums, ascending                     (batchnorm.hip 126-127; colsum.hip 61-62)"""
    return cdiv(p.rows_per_block, p.L) + p.L + cdiv(p.nblocks, 32) + 32


def depth_stats(tile_rows, nparts):
    """Epilogue statistics of mi_conv_gemm_stats: rows of one conv tile + 8 + 32 + nsplit.
      tile_rows   (32 * MT of mi_conv_gemm_plan) bounds the chain inside the conv epilogue: a lane adds its MT pixels, then 4 butterfly steps over the
                  16 lanes of a DPP row (igemm_common.h 247-253 and 266-268) - MT + 4 additions, far below the tile's row count
      + 8         bn_reduce_stage1_kernel: thread (q, l) adds rows l, l + 32, ... of its BN_RED_ROWS = 256 rows: 256 / 32  (batchnorm.hip 245-248)
      + 32        its lane order 0..31 in LDS                                                                              (batchnorm.hip 256)
      + nsplit    bn_reduce_stage2_kernel adds the nsplit = ceil(nparts / 256) splits, ascending                           (batchnorm.hip 268-271)"""
    return tile_rows + 8 + 32 + cdiv(nparts, 256)


def sum_bar(d, k, A):
    """bar[c] = 2 * (depth + k) * 2^-24 * A[c] (module docstring)."""
    return 2.0 * (d + k) * U32 * A


# ---------------------------------------------------------------------------------------------- the terms of each reduction
# k = fp32 roundings inside one term: 0 for y itself (bf16 -> fp32 is exact), 1 for y - pilot, 2 for (y - mean)^2 (the difference, the square),
# 3 for g * ((y - mean) * invstd) (batchnorm.hip 44-66).
K_OF = {"sum": (0,), "var": (2,), "pilot": (1, 2), "bwd": (0, 3), "colsum": (0,)}


def _np(t, dt):
    if torch.is_tensor(t):
        t = t.detach().cpu().to(torch.float64).numpy()          # bf16 / fp32 / bool -> float64 is exact
    return np.asarray(t).astype(dt, copy=False)


def terms(mode, dt, y, vec=None, g=None, invstd=None, keep=None):
    """The [M, C] terms of a reduction in dtype dt (np.float64: the reference; np.float32: the kernel's own arithmetic, one rounding per operation) from the
    bf16 / fp32 operands the kernel gets.  vec: mean or pilot; keep: bool [M, C], the unpacked ReLU sign bits (the reference masks g itself)."""
    y = _np(y, dt).reshape(-1, y.shape[-1])
    if mode in ("sum", "colsum"):
        return (y,)
    mu = _np(vec, dt)
    d = y - mu
    if mode == "var":
        return (d * d,)
    if mode == "pilot":
        return (d, d * d)
    gg = _np(g, dt).reshape(y.shape)
    if keep is not None:
        gg = np.where(_np(keep, dt).reshape(y.shape) > 0, gg, dt(0))
    return (gg, gg * (d * _np(invstd, dt)))


def reference(mode, p_depth, y, vec=None, g=None, invstd=None, keep=None):
    """[(ref[c], bar[c])] per output of the reduction, float64."""
    out = []
    for t, k in zip(terms(mode, np.float64, y, vec, g, invstd, keep), K_OF[mode]):
        out.append((t.sum(0), sum_bar(p_depth, k, np.abs(t).sum(0))))
    return out


def emulate(term, p, drop=None, twice_last=False, swap=None, stride=32):
    """The kernels' summation order on [M, C] fp32 terms, in numpy float32: rows per lane in row order, then lanes ascending, then the block partials strided by
    32, then the 32 lane sums ascending.  (Rows a lane does not have are added as +0, which changes nothing.)
    drop: this row is left out; twice_last: the last row is counted twice (its term doubled: exact in fp32); swap = (a, b): the results of the 8-channel slots a
    and b change places (a thread that reads the wrong slot)."""
    term = np.asarray(term, np.float32)
    M, C = term.shape
    T = cdiv(p.rows_per_block, p.L)
    full = np.zeros((p.nblocks * p.rows_per_block, C), np.float32)
    full[:M] = term
    if drop is not None:
        full[drop] = 0
    if twice_last:
        full[M - 1] *= np.float32(2)
    full = full.reshape(p.nblocks, p.rows_per_block, C)
    if T * p.L != p.rows_per_block:
        full = np.concatenate([full, np.zeros((p.nblocks, T * p.L - p.rows_per_block, C), np.float32)], 1)
    full = full.reshape(p.nblocks, T, p.L, C)
    acc = np.zeros((p.nblocks, p.L, C), np.float32)
    for t in range(T):
        acc += full[:, t]
    part = np.zeros((p.nblocks, C), np.float32)
    for q in range(p.L):
        part += acc[:, q]
    lanes = np.zeros((stride, C), np.float32)
    for b in range(p.nblocks):
        lanes[b % stride] += part[b]
    out = np.zeros(C, np.float32)
    for q in range(stride):
        out += lanes[q]
    if swap is not None:
        a, b = swap
        out = out.copy()
        out[8 * a:8 * a + 8], out[8 * b:8 * b + 8] = out[8 * b:8 * b + 8].copy(), out[8 * a:8 * a + 8].copy()
    return out


# ---------------------------------------------------------------------------------------------- per-element references
def apply_reference(y, mean, scale, beta, res=None, relu=False):
    """bn_apply_kernel (batchnorm.hip 154-157): t = ((y - mean) * scale + beta) (+ res), relu, ONE bf16 rounding.  float64 from the fp32 vectors the kernel
    receives.  bar = 2^-8 |ref| (the bf16 rounding) + 8 * 2^-24 * (|y - mean| |scale| + |beta| + |res|): the fp32 roundings of the terms that cancel (the
    difference, the product, two additions: at most 4 on any term)."""
    C = y.shape[-1]
    yy = _np(y, np.float64).reshape(-1, C)
    d, s, b = yy - _np(mean, np.float64), _np(scale, np.float64), _np(beta, np.float64)
    t = d * s + b
    mag = np.abs(d) * np.abs(s) + np.abs(b)
    if res is not None:
        r = _np(res, np.float64).reshape(-1, C)
        t, mag = t + r, mag + np.abs(r)
    if relu:
        t = np.maximum(t, 0.0)
    return t, UBF * np.abs(t) + 8 * U32 * mag


def bwd_apply_reference(g, y, mean, invstd, gamma, dbeta, dgamma, count, keep=None):
    """bn_bwd_apply_kernel (batchnorm.hip 186-188): dy = gamma * invstd * (g - dbeta * ic - xhat * dgamma * ic), xhat = (y - mean) * invstd, ic the fp32 1 / count
    the kernel is handed.  bar = 2^-8 |ref| + 8 * 2^-24 * |gamma invstd| (|g| + |dbeta ic| + |xhat dgamma ic|): at most 7 fp32 roundings touch the last term
    (difference, three products, the subtraction, gamma * invstd, the final product)."""
    C = y.shape[-1]
    ic = float(np.float32(1.0 / count))
    yy, gg = _np(y, np.float64).reshape(-1, C), _np(g, np.float64).reshape(-1, C)
    if keep is not None:
        gg = np.where(_np(keep, np.float64).reshape(-1, C) > 0, gg, 0.0)
    mu, iv, ga, db, dg = (_np(v, np.float64) for v in (mean, invstd, gamma, dbeta, dgamma))
    xhat = (yy - mu) * iv
    t2, t3 = db * ic, xhat * dg * ic
    ref = ga * iv * (gg - t2 - t3)
    return ref, UBF * np.abs(ref) + 8 * U32 * np.abs(ga * iv) * (np.abs(gg) + np.abs(t2) + np.abs(t3))


def finalize_reference(s1, s2, pilot, count, gamma, beta, eps, momentum=None, running_mean=None, running_var=None):
    """bn_finalize_channel (batchnorm.hip 208-224) in float64 from the fp32 s1, s2, pilot, gamma, beta (eps and momentum are floats there).
    Returns dict name -> ref (mean, var, invstd, scale, shift_terms = |beta| + |mean * scale|, running_mean, running_var)."""
    s1, s2, pilot, gamma, beta = (_np(v, np.float64) for v in (s1, s2, pilot, gamma, beta))
    eps = float(np.float32(eps))
    d = s1 / float(count)
    mean = pilot + d
    var = np.maximum(s2 / float(count) - d * d, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    r = dict(mean=mean, var=var, invstd=invstd, scale=gamma * invstd, shift=beta - mean * gamma * invstd,
             shift_terms=np.abs(beta) + np.abs(mean * gamma * invstd))
    if running_mean is not None:
        m = float(np.float32(momentum))
        unb = count / (count - 1.0) if count > 1 else 1.0
        r["running_mean"] = (1.0 - m) * _np(running_mean, np.float64) + m * mean
        r["running_var"] = (1.0 - m) * _np(running_var, np.float64) + m * var * unb
    return r


# ---------------------------------------------------------------------------------------------- test data
EPS = 1e-5


def channel_scale(C):
    """scale[c] = 2^((5c mod 13) - 6): neighbouring channels and neighbouring 8-channel slots differ by orders of magnitude."""
    c = np.arange(C)
    return 2.0 ** ((5 * c) % 13 - 6)


BN_CHANNELS = (8, 24, 48, 64, 264, 1048, 2048)          # L = 256, 64, 32, 32, 4, 1, 1; all but 8, 64 and 2048 leave slots of cp idle


def bn_shapes():
    """(C, M): the smallest M that reach each edge of bn_plan and of the row loop for every L: one row, L - 1, L, L + 1 (a block of one row), 3L + 1, 4L,
    4L + 1, 256 L and 256 L + 1 (256 full blocks; rows_per_block grows to 2L and the last block holds ONE row), 33 * 7 * L + 5 (231 blocks and a part: a
    block count that is no multiple of 32).
    Correction to the issue's list, from the code: bn_plan cuts M into up to 256 blocks BEFORE the row loop runs, so up to M = 256 L a block has L rows - one
    per lane - and `r + 3 * lanes < r1` (batchnorm.hip 72) is false for every lane: 3L + 1, 4L and 4L + 1 are block-count cases, the four-row trip is not
    reached below rows_per_block = 4L, i.e. M > 768 L.  Four more M per C reach it: 1024 L (rows_per_block 4L: one trip, no tail), 1024 L + 1 (5L: a trip,
    then one tail row), 1792 L (7L: a trip and three tail rows; lane 0 ends the trip loop on r + 3L == r1 exactly) and 2048 L (8L: two trips)."""
    out = []
    for C in BN_CHANNELS:
        L = plan(1, C).L
        ms = [1, L - 1, L, L + 1, 3 * L + 1, 4 * L, 4 * L + 1, 256 * L, 256 * L + 1, 33 * 7 * L + 5, 1024 * L, 1024 * L + 1, 1792 * L, 2048 * L]
        seen = []
        for m in ms:
            if m > 0 and m not in seen:
                seen.append(m)
        out += [(C, m) for m in seen]
    return out


def make_bn_case(C, M, variant="std"):
    """Operands of one (C, M) case, on the CPU.  y, g, res bf16 [M, C]; mean, pilot, invstd, gamma, beta fp32 [C]; keep bool [M, C] (60 % kept).
    variant "pilot0": the pilot is exactly zero; "const": channel 5 is constant (variance exactly 0)."""
    gen = torch.Generator().manual_seed(1000 * C + M)
    sc = torch.from_numpy(channel_scale(C)).float()
    mu = 3.0 * sc * torch.sin(torch.arange(C).float())
    y = (torch.randn(M, C, generator=gen) * sc + mu).to(torch.bfloat16)
    if variant == "const":
        y[:, 5] = 0.75 * sc[5]
    g = (torch.randn(M, C, generator=gen) * sc.flip(0)).to(torch.bfloat16)
    res = (torch.randn(M, C, generator=gen) * sc).to(torch.bfloat16)
    keep = torch.rand(M, C, generator=gen) < 0.6
    y64 = y.double()
    true_mean = y64.mean(0)
    true_var = ((y64 - true_mean) ** 2).mean(0)
    # the vectors the kernels are handed.  mean: within half a sigma of the batch mean, NOT the mean itself (at M = 1 every (y - mean)^2 would be exactly 0 and
    # the check of that sum blind); the references use the same fp32 vector, so nothing of the statistics' own error enters
    mean = (true_mean + 0.5 * sc.double() * torch.sin(2.0 * torch.arange(C).double() + 1.0)).float()
    invstd = torch.rsqrt(true_var + EPS).float()
    # pilot: within one sigma of the true mean (the running mean in training)
    pilot = (true_mean + sc.double() * torch.cos(3.0 * torch.arange(C).double())).float()
    if variant == "pilot0":
        pilot = torch.zeros(C)
    if variant == "const":
        pilot[5] = y[0, 5].float() - 8.0
    gamma = (0.5 + torch.rand(C, generator=gen)) * sc.roll(3)
    beta = torch.randn(C, generator=gen) * sc.roll(5)
    return dict(C=C, M=M, y=y, g=g, res=res, keep=keep, mean=mean, invstd=invstd, pilot=pilot, gamma=gamma.float(), beta=beta.float())


def make_int_case(C, M):
    """Integer-valued operands: y, g in [-a, a], mean / pilot in [-a / 2, a / 2], invstd ONE power of two per channel (2^-2 .. 2^1).  With a = 8,
    |y - mean| <= 12: every term of channel c is an integer multiple of its unit (1, or invstd[c] for g * xhat) of at most 144 units ((y - mean)^2;
    |g (y - mean)| <= 96), and every partial sum stays below 2^24 units up to M = 65537 (65537 * 144 < 2^24): the fp32 sums are exact in ANY order.  The
    larger M of the four-row-trip shapes take a = 2 (at most 9 units a term: 524 288 * 9 < 2^24)."""
    a = 8 if M * 144 < 2 ** 24 else 2
    assert M * (a + a // 2) ** 2 < 2 ** 24
    gen = torch.Generator().manual_seed(7000 * C + M)
    y = torch.randint(-a, a + 1, (M, C), generator=gen).to(torch.bfloat16)
    g = torch.randint(-a, a + 1, (M, C), generator=gen).to(torch.bfloat16)
    mean = torch.randint(-a // 2, a // 2 + 1, (C,), generator=gen).float()
    invstd = (2.0 ** (torch.arange(C) % 4 - 2).double()).float()
    keep = torch.rand(M, C, generator=gen) < 0.6
    return dict(C=C, M=M, y=y, g=g, mean=mean, invstd=invstd, keep=keep)


def pack_bits(keep):
    """bool [M, C] -> the packed sign bits the kernels read: int16 [M, C / 16], bit c % 16 of word c / 16."""
    M, C = keep.shape
    w = (keep.view(M, C // 16, 16).to(torch.int32) << torch.arange(16, dtype=torch.int32)).sum(-1)
    return torch.from_numpy(w.numpy().astype(np.uint16).view(np.int16).copy())


def unpack_bits(bits, C):
    """int16 [..., C / 16] -> bool [M, C]."""
    b = bits.contiguous().view(torch.uint8).reshape(-1, C // 8).to(torch.int32)
    return ((b[..., None] >> torch.arange(8, dtype=torch.int32, device=b.device)) & 1).reshape(-1, C).bool()


# ---------------------------------------------------------------------------------------------- colsum.hip
ASPP_K = (1, 19, 21, 256)
BIAS_N = (8, 48, 1048, 2048)


def colsum_shapes(widths, vec):
    """(N, M) with M in {1, 8L - 1, 8L, 8L + 1 (the minimum block height: one block | two blocks, the second of one row), 512 * 8L + 1 (the 512-block cap: rows
    grows to 8L + 1, which is no multiple of L)}.  The 512-block cap cannot be reached with less: at L = 256 (K = 1 fp32, N = 8 bf16) that is
    M = 1 048 577 rows, 4 MB and 16 MB of input - above the few MB of every other case, and still milliseconds on the device."""
    out = []
    for N in widths:
        L = colsum_plan(1, N, vec).L
        out += [(N, m) for m in (1, 8 * L - 1, 8 * L, 8 * L + 1, 512 * 8 * L + 1)]
    return out


def make_colsum_case(N, M, bf16):
    gen = torch.Generator().manual_seed(31 * N + M)
    sc = torch.from_numpy(channel_scale(N)).float()
    x = torch.randn(M, N, generator=gen) * sc + 0.5 * sc * torch.sin(torch.arange(N).float())
    return x.to(torch.bfloat16) if bf16 else x


def make_colsum_int_case(N, M, bf16):
    """Integers in [-8, 8]: every partial sum is an integer below 2^24 (1 048 577 * 8 < 2^24): exact in any order."""
    gen = torch.Generator().manual_seed(77 * N + M)
    x = torch.randint(-8, 9, (M, N), generator=gen)
    return x.to(torch.bfloat16) if bf16 else x.float()
