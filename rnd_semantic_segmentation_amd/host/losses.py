"""The binary-segmentation loss family of the reference's attention model (core/models/classifiers/attn/loss.py) on the HIP kernels:

  TverskyLoss(alpha=0.7, eps=1)      loss.py:7-27     1 - (TP + eps) / (TP + alpha FN + (1 - alpha) FP + eps), sums over the whole batch
  BinaryCrossEntropyLoss()           loss.py:66-74    F.binary_cross_entropy_with_logits(pred, label.float())
  CompoundLoss(losses, weights)      loss.py:42-64    sum_i w_i loss_i(*inputs), default weights 1 / N
  MultiscaleLoss(loss_fn)            loss.py:29-40    sum over zip(predicts, labels)
  BoundaryLoss(thresh=0.5)           not in the reference: Kervadec et al. (MIDL 2019), mean(sigmoid(pred) * phi(label)), phi the signed distance map of
                                     (label >= thresh) from mi_signed_distance; in a CompoundLoss it is the `rest` kind of term, a call of its own

The first four run one autograd Function over mi_upsample_tversky_bce at the identity scale (h == H, w == W: every interpolation weight is 0), whose two
weights select the terms; a CompoundLoss of Tversky and BCE terms folds its weights into ONE call.  Inputs: pred [B,1,H,W] or [B,H,W] logits and a label
of the same shape with values in [0, 1], both on the GPU; CPU tensors and more than one channel are refused (the reference sums dims [0, 2, 3] per channel;
every user here has one).  PraNetTrainer does not go through these modules: PraNet.losses() runs the fused kernel on the low-resolution maps.
"""
import torch
import torch.nn as nn

from .. import kernels as K


class _TverskyBceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, alpha, eps, w_tversky, w_bce):
        B, H, W = pred.shape[0], pred.shape[-2], pred.shape[-1]
        out, d, _ = K.upsample_tversky_bce(pred.contiguous().view(B, H, W), label.contiguous().view(B, H, W), want_grad=ctx.needs_input_grad[0],
                                           alpha=alpha, eps=eps, weights=(w_tversky, w_bce), align_corners=False)
        ctx.d, ctx.shape = d, pred.shape
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, gout, _gterms):
        d, ctx.d = ctx.d, None
        return (d * gout).view(ctx.shape), None, None, None, None, None


def tversky_bce(pred, label, alpha=0.7, eps=1.0, weights=(0.5, 0.5), with_terms=False):
    """weights[0] * TverskyLoss(alpha, eps)(pred, label) + weights[1] * BinaryCrossEntropyLoss()(pred, label) in one kernel call; the gradient flows to
    pred only and `label` is left as it is.  with_terms=True also returns the call's float32 [4] device tensor loss, tversky, bce, 0."""
    who = "the Tversky / BCE losses"
    if not (pred.is_cuda and label.is_cuda):
        raise NotImplementedError("%s run on the MI355X only (got %s / %s tensors): no CPU path exists" % (who, pred.device, label.device))
    if pred.dim() not in (3, 4) or (pred.dim() == 4 and pred.shape[1] != 1):
        raise NotImplementedError("%s take one-channel logits [B,1,H,W] or [B,H,W] (got %s: C > 1 is not implemented)" % (who, tuple(pred.shape)))
    if tuple(label.shape) != tuple(pred.shape):
        raise ValueError("%s: label %s does not match pred %s" % (who, tuple(label.shape), tuple(pred.shape)))
    if not 0.0 <= float(alpha) <= 1.0 or not float(eps) > 0.0:
        raise ValueError("%s: alpha in [0, 1] and eps > 0, got %r / %r" % (who, alpha, eps))
    loss, terms = _TverskyBceFn.apply(pred.float(), label.float(), float(alpha), float(eps), float(weights[0]), float(weights[1]))
    return (loss, terms) if with_terms else loss


class _BoundaryFn(torch.autograd.Function):
    """mean(sigmoid(pred) * phi) over every pixel, d / d pred = phi p (1 - p) / N; phi is a constant of the label."""

    @staticmethod
    def forward(ctx, pred, phi):
        p = torch.sigmoid(pred)
        ctx.save_for_backward(p, phi)
        return (p * phi).mean()

    @staticmethod
    def backward(ctx, gout):
        p, phi = ctx.saved_tensors
        return (phi * p * (1.0 - p)) * (gout / p.numel()), None


def boundary(pred, label, thresh=0.5):
    """The boundary loss on materialised logits: mean(sigmoid(pred) * phi(label)); the gradient flows to pred only and `label` is left as it is."""
    who = "the boundary loss"
    if not (pred.is_cuda and label.is_cuda):
        raise NotImplementedError("%s runs on the MI355X only (got %s / %s tensors): no CPU path exists" % (who, pred.device, label.device))
    if pred.dim() not in (3, 4) or (pred.dim() == 4 and pred.shape[1] != 1):
        raise NotImplementedError("%s takes one-channel logits [B,1,H,W] or [B,H,W] (got %s: C > 1 is not implemented)" % (who, tuple(pred.shape)))
    if tuple(label.shape) != tuple(pred.shape):
        raise ValueError("%s: label %s does not match pred %s" % (who, tuple(label.shape), tuple(pred.shape)))
    B, H, W = label.shape[0], label.shape[-2], label.shape[-1]
    phi = K.signed_distance(label.detach().float().contiguous().view(B, H, W), thresh)
    return _BoundaryFn.apply(pred.float(), phi.view(pred.shape))


class BoundaryLoss(nn.Module):
    def __init__(self, thresh=0.5):
        super().__init__()
        self.thresh = thresh

    def forward(self, pred, label):
        return boundary(pred, label, self.thresh)


class TverskyLoss(nn.Module):
    def __init__(self, alpha=0.7, eps=1):
        super().__init__()
        self.eps = eps
        self.alpha = alpha

    def forward(self, pred, label):
        return tversky_bce(pred, label, self.alpha, self.eps, (1.0, 0.0))


class BinaryCrossEntropyLoss(nn.Module):
    def forward(self, pred, label):
        return tversky_bce(pred, label, weights=(0.0, 1.0))


class CompoundLoss(nn.Module):
    def __init__(self, losses, weights=None):
        super().__init__()
        if weights is None:
            N = len(losses)
            weights = [1. / N] * N
        self.weights = weights
        self.losses = nn.ModuleList(losses)

    def forward(self, *inputs):
        """sum_i w_i loss_i(*inputs).  The Tversky terms that share (alpha, eps) and every BCE term become one kernel call with their weights added up;
        any other module is called as it is."""
        calls, bce, rest = {}, 0.0, []
        for fn, w in zip(self.losses, self.weights):
            if type(fn) is TverskyLoss:
                calls[(fn.alpha, fn.eps)] = calls.get((fn.alpha, fn.eps), 0.0) + w
            elif type(fn) is BinaryCrossEntropyLoss:
                bce += w
            else:
                rest.append((fn, w))
        if bce and not calls:
            calls[(0.7, 1)] = 0.0
        loss = None
        for i, ((alpha, eps), w) in enumerate(calls.items()):
            term = tversky_bce(*inputs, alpha=alpha, eps=eps, weights=(w, bce if i == 0 else 0.0))
            loss = term if loss is None else loss + term
        for fn, w in rest:
            term = w * fn(*inputs)
            loss = term if loss is None else loss + term
        if loss is None:
            return torch.scalar_tensor(0, device=torch.device("cuda" if torch.cuda.is_available() else "cpu"))
        return loss


class MultiscaleLoss(nn.Module):
    def __init__(self, loss_fn):
        super().__init__()
        self.loss_fn = loss_fn

    def forward(self, predicts, labels):
        loss = None
        for pred, label in zip(predicts, labels):
            term = self.loss_fn(pred, label)
            loss = term if loss is None else loss + term
        if loss is None:
            return torch.scalar_tensor(0, device=torch.device("cuda" if torch.cuda.is_available() else "cpu"))
        return loss
