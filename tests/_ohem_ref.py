"""Float64 restatement of the cross-entropy with online hard example mining (OHEM) on bilinearly upsampled logits, with its gradient written out, a
second function that takes loss and gradient from F.cross_entropy on the kept pixels by autograd, and the case table of tests/test_host_ohem.py /
tests/test_gpu_ohem.py.

    z = bilinear(low), p = softmax(z), y = label, valid = label not ignore_index and inside [0, K), q_i = p_i[y_i] on valid pixels, n their count
    k      = min(min_kept, n)
    t      = max(thresh, k-th smallest q over the valid pixels)          (1-based; n == 0: t = thresh)
    kept_i = valid_i and q_i <= t
    loss   = sum_kept (-log q_i) / n_kept
    dl/dz_c at pixel i = kept_i (p_i[c] - [c == y_i]) / n_kept;  d loss / d low = the transposed bilinear of that
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from _wce_ref import SHAPE_BY_NAME, Shape, make_inputs

OhemRef = collections.namedtuple("OhemRef", "loss n_kept t bad dlow q margin kept")          # dlow [B,h,w,K]; q [B,H,W] (2.0 where not valid)
SENTINEL = 2.0


def _low64(low):
    return torch.as_tensor(np.array(low)).double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)


def _upsampled(low, labels, align_corners):
    x = _low64(low)
    lab = torch.as_tensor(np.array(labels)).long()
    return x, lab, F.interpolate(x, size=tuple(lab.shape[-2:]), mode="bilinear", align_corners=align_corners)


def ohem_ref(low, labels, thresh, min_kept, align_corners=True, ignore_index=255):
    """low [B,h,w,K], labels [B,H,W] int64 -> OhemRef in float64.  margin: the smallest |q_i - t| / t over the valid pixels with q_i != t (inf if
    there is none)."""
    x, lab, z = _upsampled(low, labels, align_corners)
    K = x.shape[1]
    zd = z.detach()
    lp = zd - zd.max(1, keepdim=True).values
    lp = lp - torch.log(torch.exp(lp).sum(1, keepdim=True))
    p = torch.exp(lp)
    valid = (lab != ignore_index) & (lab >= 0) & (lab < K)
    bad = int(((lab != ignore_index) & ~valid).sum())
    y = torch.where(valid, lab, torch.zeros_like(lab))
    onehot = F.one_hot(y, K).permute(0, 3, 1, 2).double()
    q = (p * onehot).sum(1)
    nll = -(lp * onehot).sum(1)
    n = int(valid.sum())
    k = min(int(min_kept), n)
    t = float(thresh)
    if k > 0:
        t = max(t, float(torch.sort(q[valid]).values[k - 1]))
    kept = valid & (q <= t)
    n_kept = int(kept.sum())
    loss = nll[kept].sum() / n_kept if n_kept else torch.tensor(float("nan"), dtype=torch.float64)
    dz = kept.double().unsqueeze(1) * (p - onehot) / max(n_kept, 1)
    dlow, = torch.autograd.grad(z, x, dz)
    qv = q[valid]
    off = qv[qv != t]
    margin = float(((off - t).abs() / t).min()) if off.numel() and t > 0 else float("inf")
    q_out = torch.where(valid, q, torch.full_like(q, SENTINEL))
    return OhemRef(loss, n_kept, t, bad, dlow.permute(0, 2, 3, 1).contiguous(), q_out, margin, kept)


def ohem_autograd(low, labels, kept, align_corners=True, ignore_index=255):
    """(loss, dlow [B,h,w,K]) in float64 from F.cross_entropy(z, where(kept, label, ignore)) by autograd: the mean over the kept pixels."""
    x, lab, z = _upsampled(low, labels, align_corners)
    loss = F.cross_entropy(z, torch.where(kept, lab, torch.full_like(lab, ignore_index)), ignore_index=ignore_index)
    loss.backward()
    return loss.detach(), x.grad.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the cases
# A case: a shape of _wce_ref.SHAPES (or one added here), a setting, and how its inputs are made.  min_kept is given from the n valid pixels ("div", d: max(1, n // d);
# "mul", m: n m) or as a number ("abs", m).  salt: appended to the input key until the case meets the margin condition of
# tests/test_host_ohem.py (a condition on the inputs, never on the kernel).
Case = collections.namedtuple("Case", "name shape thresh kind amount magnitude constant salt")
GEOMETRY = ("one", "1x1_5x3", "ident_ac", "ident", "k19_ac", "k19", "k32", "tiles_ac", "tiles", "f32")
MANY_WG = Shape("many_wg", 2, 19, (12, 16), (96, 128), False)          # 24 576 pixels: 96 workgroups of the streaming passes, 4 of the probability pass
# the streaming passes (histogram levels 1 and 2, loss) run at most 1024 workgroups of 256 threads: above 262 144 pixels a workgroup takes a second trip
SECOND_TRIP = Shape("second_trip", 1, 3, (8, 8), (513, 512), True)
SETTINGS = (("minkept", 0.05, "div", 3), ("thresh", 0.7, "abs", 1), ("all", 0.0, "mul", 10))

# salts found by tests/test_host_ohem.py's margin condition (0 = the plain key)
_SALTS = {"tiles-minkept": 1, "cluster": 5, "many_wg": 1}


def _cases():
    out = []
    for g in GEOMETRY:
        for sname, thresh, kind, amount in SETTINGS:
            name = "%s-%s" % (g, sname)
            out.append(Case(name, SHAPE_BY_NAME[g], thresh, kind, amount, None, False, _SALTS.get(name, 0)))
    k19 = SHAPE_BY_NAME["k19"]
    # every q within a relative 1e-3 of 1/19: the k-th smallest is found on the last radix level only.  thresh 0, min_kept 1: t is the smallest q
    out.append(Case("cluster", k19, 0.0, "abs", 1, 1e-3, False, _SALTS.get("cluster", 0)))
    out.append(Case("ties", k19, 0.0, "div", 2, None, True, 0))                                    # constant logits: every q equal, all kept
    out.append(Case("many_wg", MANY_WG, 0.001, "div", 3, None, False, _SALTS.get("many_wg", 0)))
    out.append(Case("second_trip", SECOND_TRIP, 0.0, "abs", 64, None, False, _SALTS.get("second_trip", 0)))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
PARITY_BAR = 2e-5          # the fused heads' bar (tests/test_gpu_wce.py, tests/test_gpu_gdl.py)
MARGIN = 1e-4              # five times the bar: a kernel within its bar cannot move a pixel across t


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(low, labels, thresh, min_kept) of a case; cached, never modified by a test."""
    c = CASE_BY_NAME[name]
    s = c.shape
    key = "ohem.%s" % s.name + (".%d" % c.salt if c.salt else "")
    low, lab = make_inputs(key, s.B, s.K, s.hw, s.HW, magnitude=c.magnitude)
    if c.constant:
        low = np.full_like(low, 0.25)
    n = int(((lab != 255) & (lab >= 0) & (lab < s.K)).sum())
    min_kept = {"div": max(1, n // c.amount), "mul": max(1, n * c.amount), "abs": c.amount}[c.kind]
    low.setflags(write=False)
    lab.setflags(write=False)
    return low, lab, c.thresh, min_kept


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """The float64 expectation of a case, computed once and shared."""
    low, lab, thresh, min_kept = case_inputs(name)
    return ohem_ref(low, lab, thresh, min_kept, CASE_BY_NAME[name].shape.align_corners)
