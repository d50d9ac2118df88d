"""One GaldFada iteration composed from the oracle's CPU modules (oracle/ref_gald.py: GCPAEncoder / GCPADecoder, oracle/ref_model.py:
RefPixelDiscriminator) and torch.optim.Adam, fp32 - the reference's core/combos/gald_fada.py:69-136 line by line.  Test infrastructure for
tests/test_gpu_gald_fada.py: returns the four losses, every gradient as it stands when its optimizer steps, and leaves the modules stepped."""
import torch
import torch.nn.functional as F

from oracle import ref_model


def poly(base_lr, it, max_iter, power=0.9):
    """core/utils/adapt_lr.py adjust_learning_rate('poly')."""
    return base_lr * ((1 - float(it) / max_iter) ** power)


def make_optimizers(renc, rdec, rD, base_lr, base_lr_d):
    """gald_trainer.py (Adam, encoder lr / decoder 10 x lr) and fada_adapter.py:24 (Adam, betas (0.9, 0.99))."""
    return (torch.optim.Adam(renc.parameters(), lr=base_lr), torch.optim.Adam(rdec.parameters(), lr=base_lr * 10),
            torch.optim.Adam(rD.parameters(), lr=base_lr_d, betas=(0.9, 0.99)))


def _grads(mod, tag):
    return {"%s.%s" % (tag, k): p.grad.detach().clone().numpy() for k, p in mod.named_parameters() if p.grad is not None}


def gald_fada_step(renc, rdec, rD, opts, src, label, tgt, iteration, max_iter, base_lr, base_lr_d, T=1.8, autocast=False):
    opt_enc, opt_dec, opt_D = opts
    iteration += 1                                                          # gald_fada.py:69
    lr, lr_d = poly(base_lr, iteration, max_iter), poly(base_lr_d, iteration, max_iter)
    for g in opt_enc.param_groups:
        g["lr"] = lr
    for g in opt_dec.param_groups:
        g["lr"] = lr * 10
    for g in opt_D.param_groups:
        g["lr"] = lr_d
    for o in opts:
        o.zero_grad()                                                       # (set_to_none: linear5/4/3 keep .grad None)
    src_size, tgt_size = src.shape[-2:], tgt.shape[-2:]
    out = {}

    def run(fn):
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                return fn()
        return fn()

    src_feats = run(lambda: renc(src))                                      # :79-81
    src_output = run(lambda: rdec(src, src_feats))[-1].float().div(T)
    loss_seg = F.cross_entropy(src_output, label, ignore_index=255)          # :85-88
    loss_seg.backward()
    src_soft = F.softmax(src_output, dim=1).detach()                         # :91-92
    src_soft[src_soft > 0.9] = 0.9
    tgt_feats = run(lambda: renc(tgt))                                      # :94-96
    tgt_output = run(lambda: rdec(tgt, tgt_feats))[-1].float().div(T)
    tgt_soft = F.softmax(tgt_output, dim=1).detach()                         # :100-102
    tgt_soft[tgt_soft > 0.9] = 0.9
    tgt_D = run(lambda: rD(tgt_feats[3], tgt_size)).float()                # :104-105
    loss_adv_tgt = 0.001 * ref_model.ref_soft_label_cross_entropy(tgt_D, torch.cat((tgt_soft, torch.zeros_like(tgt_soft)), dim=1))
    loss_adv_tgt.backward()
    out["grads_gen"] = {**_grads(renc, "enc"), **_grads(rdec, "dec")}       # as they stand at :108-109
    opt_enc.step()
    opt_dec.step()
    opt_D.zero_grad()                                                       # :111
    src_D = run(lambda: rD(src_feats[3].detach(), src_size)).float()        # :113-115
    loss_D_src = 0.5 * ref_model.ref_soft_label_cross_entropy(src_D, torch.cat((src_soft, torch.zeros_like(src_soft)), dim=1))
    loss_D_src.backward()
    tgt_D = run(lambda: rD(tgt_feats[3].detach(), tgt_size)).float()        # :117-119
    loss_D_tgt = 0.5 * ref_model.ref_soft_label_cross_entropy(tgt_D, torch.cat((torch.zeros_like(tgt_soft), tgt_soft), dim=1))
    loss_D_tgt.backward()
    out["grads_D"] = _grads(rD, "D")                                        # as they stand at :121
    opt_D.step()
    out["losses"] = [float(loss_seg), float(loss_adv_tgt), float(loss_D_src), float(loss_D_tgt)]
    out["lr"], out["lr_d"] = lr, lr_d
    return out


def adversarial_grads(renc, rdec, rD, tgt, T=1.8, autocast=False):
    """The target pass's adversarial term alone (gald_fada.py:94-106): d(0.001 * soft_label_cross_entropy(model_D(feats[3], size),
    cat(soft, 0))) / d(encoder parameters).  Returns (loss, encoder gradients, decoder gradients - none: the soft labels are detached)."""
    for m in (renc, rdec, rD):
        m.zero_grad(set_to_none=True)

    def run(fn):
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                return fn()
        return fn()

    feats = run(lambda: renc(tgt))
    tgt_output = run(lambda: rdec(tgt, feats))[-1].float().div(T)
    soft = F.softmax(tgt_output, dim=1).detach()
    soft[soft > 0.9] = 0.9
    pred = run(lambda: rD(feats[3], tgt.shape[-2:])).float()
    loss = 0.001 * ref_model.ref_soft_label_cross_entropy(pred, torch.cat((soft, torch.zeros_like(soft)), dim=1))
    loss.backward()
    return float(loss), _grads(renc, "enc"), _grads(rdec, "dec")
