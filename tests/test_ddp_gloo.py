"""Data-parallel path on CPU: world_size 2, gloo backend (what runs over RCCL on the 8-GPU node).
Checks (1) bucket construction, (2) GradAllReducer gives the cross-rank average of the per-rank gradients,
(3) an ASPPTrainer step in a 2-rank job equals a single-process step on the averaged gradient, on every rank."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _cases
from oracle import ref_model
from rnd_semantic_segmentation_amd.host import config as hc
from rnd_semantic_segmentation_amd.host import ddp, engine, synth


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _models():
    fe, cls = ref_model.RefFeatureExtractor((1, 1, 1, 1)), ref_model.RefASPP()
    synth.load_formula_weights(fe)
    synth.load_formula_weights(cls)
    return fe, cls


def _batch(rank):
    x, lab = _cases.net_inputs(1, 33, 70 + rank)
    return torch.from_numpy(x), torch.from_numpy(lab)


def _cpu_only():
    """The trainers move to cuda whenever a GPU is visible (host/plugin.py); the ranks of this module test the CPU data-parallel path, on any host."""
    torch.cuda.is_available = lambda: False


def test_bucket_ranges_cover_the_store_from_the_end():
    params = [("p%d" % i, torch.nn.Parameter(torch.zeros(n))) for i, n in enumerate((1000, 64, 5000, 300, 7000, 10))]
    st = engine.FlatStore(params, torch.device("cpu"))
    red = ddp.GradAllReducer([st], bucket_bytes=4 * 6000)
    bks = red.buckets[id(st)]
    assert bks[0].hi == st.total and bks[-1].lo == 0
    for a, b in zip(bks, bks[1:]):
        assert a.lo == b.hi                                   # contiguous, descending
    assert all(b.lo in st.offsets for b in bks)               # cut at parameter boundaries
    assert all(p.grad.data_ptr() == st.grad.data_ptr() + 4 * p._mi_off for _, p in params)


def _worker(rank, world, port, tmpdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    _cpu_only()
    try:
        # (2) raw reducer
        fe, cls = _models()
        stores = [engine.FlatStore(list(cls.named_parameters()), torch.device("cpu")),
                  engine.FlatStore(list(fe.named_parameters()), torch.device("cpu"))]
        red = ddp.GradAllReducer(stores, bucket_bytes=1 << 20)
        x, lab = _batch(rank)
        for m in (fe, cls):
            for p in m.parameters():
                p.grad = None                                  # as a foreign optimizer's zero_grad would leave it
        loss = torch.nn.functional.cross_entropy(cls(fe(x), lab.shape[-2:]), lab.long(), ignore_index=255)
        loss.backward()
        red.finish()
        np.save(os.path.join(tmpdir, "grad_cls_%d.npy" % rank), stores[0].grad.numpy())
        np.save(os.path.join(tmpdir, "grad_fe_%d.npy" % rank), stores[1].grad.numpy())
        # (3) trainer step in a distributed job
        from rnd_semantic_segmentation_amd.host import trainer as tr
        cfg = hc.CfgNode(hc.default_tree())
        cfg.merge_from_list(["MODEL.NUM_CLASSES", 19, "MODEL.FREEZE_BN", True, "SOLVER.BASE_LR", 5e-4, "OUTPUT_DIR", tmpdir])
        cfg.freeze()

        class T(tr.ASPPTrainer):
            build_feature_extractor = staticmethod(lambda cfg: _models()[0])
            build_classifier = staticmethod(lambda cfg: _models()[1])

        import logging
        t = T("aspp", cfg, [None] * 4, rank, logger=logging.getLogger("ddp%d" % rank))
        assert t.distributed and t.world_size == 2 and t.reducer is not None
        t.train_step(x, lab, 100)
        flat = torch.cat([p.detach().reshape(-1) for p in list(t.feature_extractor.parameters()) + list(t.classifier.parameters())])
        np.save(os.path.join(tmpdir, "params_%d.npy" % rank), flat.numpy())
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_gradient_average_and_trainer_step(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    # single-process expectation: average of the two per-rank gradients (mean of per-rank mean losses)
    grads = []
    for r in range(2):
        fe, cls = _models()
        x, lab = _batch(r)
        torch.nn.functional.cross_entropy(cls(fe(x), lab.shape[-2:]), lab.long(), ignore_index=255).backward()
        grads.append({k: p.grad.clone() for m in (fe, cls) for k, p in m.named_parameters()})
    avg = {k: (grads[0][k] + grads[1][k]) / 2 for k in grads[0]}
    fe, cls = _models()
    st_cls = engine.FlatStore(list(cls.named_parameters()), torch.device("cpu"))
    st_fe = engine.FlatStore(list(fe.named_parameters()), torch.device("cpu"))
    for st, tag in ((st_cls, "cls"), (st_fe, "fe")):
        want = torch.zeros(st.total)
        for name, p in zip(st.names, st.params):
            want[p._mi_off:p._mi_off + p.numel()] = avg[name].reshape(-1)
        for r in range(2):
            got = np.load(tmp_path / ("grad_%s_%d.npy" % (tag, r)))
            assert np.abs(got - want.numpy()).max() <= 1e-6 * max(np.abs(want.numpy()).max(), 1e-12) + 1e-9
    # trainer: both ranks hold identical parameters == one SGD step on the averaged gradient
    p0, p1 = np.load(tmp_path / "params_0.npy"), np.load(tmp_path / "params_1.npy")
    assert np.array_equal(p0, p1)
    fe, cls = _models()
    of, oc = ref_model.make_optimizers(fe, cls, 5e-4)
    for m in (fe, cls):
        for k, p in m.named_parameters():
            p.grad = avg[k].clone()
    of.step()
    oc.step()
    want = torch.cat([p.detach().reshape(-1) for p in list(fe.parameters()) + list(cls.parameters())]).numpy()
    assert np.abs(p0 - want).max() <= 2e-6 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ FADA, two ranks
def _fada_models():
    fe, cls = _models()
    D = ref_model.RefPixelDiscriminator(2048, 256, 19)
    synth.load_formula_weights(D)
    return fe, cls, D


def _fada_batch(rank):
    xs = torch.from_numpy(synth.synth_image(1, 33, 33, seed=300 + rank))
    ys = torch.from_numpy(synth.synth_label(1, 33, 33, 19, seed=300 + rank))
    xt = torch.from_numpy(synth.synth_image(1, 33, 33, seed=400 + rank))
    return xs, ys, xt


def _fada_worker(rank, world, port, tmpdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    _cpu_only()
    try:
        import logging
        from rnd_semantic_segmentation_amd.host import fada
        from rnd_semantic_segmentation_amd.host import trainer as tr
        cfg = hc.CfgNode(hc.default_tree())
        cfg.merge_from_list(["MODEL.NUM_CLASSES", 19, "MODEL.FREEZE_BN", True, "SOLVER.BASE_LR", 5e-4, "SOLVER.BASE_LR_D", 1e-4,
                             "OUTPUT_DIR", tmpdir])
        cfg.freeze()
        tr.ASPPTrainer.build_feature_extractor = staticmethod(lambda cfg: _fada_models()[0])
        tr.ASPPTrainer.build_classifier = staticmethod(lambda cfg: _fada_models()[1])
        fada.FADAAdapter.build_adversarial_discriminator = staticmethod(lambda cfg: _fada_models()[2])
        fada.setup_logger = lambda *a, **k: logging.getLogger("fada_ddp%d" % rank)
        combo = fada.AsppFada("aspp_fada", cfg, [None] * 4, [None] * 4, rank)
        assert combo.aspp.reducer is not None and combo.fada.reducer is not None and combo.fada.distributed
        xs, ys, xt = _fada_batch(rank)
        r = combo.train_step(xs, ys, xt, 40)
        flat = torch.cat([p.detach().reshape(-1) for m in (combo.aspp.feature_extractor, combo.aspp.classifier, combo.fada.model_D)
                          for p in m.parameters()])
        np.save(os.path.join(tmpdir, "fada_params_%d.npy" % rank), flat.numpy())
        np.save(os.path.join(tmpdir, "fada_losses_%d.npy" % rank), np.array([float(r[k]) for k in ("loss_seg", "loss_adv_tgt", "loss_D_src", "loss_D_tgt")]))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_fada_iteration(tmp_path):
    """AsppFada in a 2-rank job: generator-side gradients (two backward passes accumulate before ONE all-reduce) and the
    discriminator's gradients are averaged over ranks, every rank ends with identical parameters, equal to a single process
    applying the averaged gradients of the oracle's literal iteration."""
    port = _free_port()
    mp.spawn(_fada_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    p0, p1 = np.load(tmp_path / "fada_params_0.npy"), np.load(tmp_path / "fada_params_1.npy")
    assert np.array_equal(p0, p1)
    # single-process expectation: run the literal iteration per rank WITHOUT optimizer steps to collect gradients at the two
    # points of the iteration (generator step, discriminator step), average them, and apply the reference's updates.
    import torch.nn.functional as F
    T = 1.8
    gen_grads, d_grads, losses = [], [], []
    for r in range(2):
        fe, cls, D = _fada_models()
        xs, ys, xt = _fada_batch(r)
        src_fea = fe(xs)
        src_pred = cls(src_fea, xs.shape[-2:]).div(T)
        loss_seg = F.cross_entropy(src_pred, ys.long(), ignore_index=255)
        loss_seg.backward()
        src_soft = F.softmax(src_pred, 1).detach()
        src_soft[src_soft > 0.9] = 0.9
        tgt_fea = fe(xt)
        tgt_soft = F.softmax(cls(tgt_fea, xt.shape[-2:]).div(T), 1).detach()
        tgt_soft[tgt_soft > 0.9] = 0.9
        loss_adv = 0.001 * ref_model.ref_soft_label_cross_entropy(D(tgt_fea, xt.shape[-2:]), torch.cat((tgt_soft, torch.zeros_like(tgt_soft)), 1))
        loss_adv.backward()
        gen_grads.append({k: p.grad.clone() for m in (fe, cls) for k, p in m.named_parameters()})
        for p in D.parameters():
            p.grad = None
        l_src = 0.5 * ref_model.ref_soft_label_cross_entropy(D(src_fea.detach(), xs.shape[-2:]), torch.cat((src_soft, torch.zeros_like(src_soft)), 1))
        l_src.backward()
        l_tgt = 0.5 * ref_model.ref_soft_label_cross_entropy(D(tgt_fea.detach(), xt.shape[-2:]), torch.cat((torch.zeros_like(tgt_soft), tgt_soft), 1))
        l_tgt.backward()
        d_grads.append({k: p.grad.clone() for k, p in D.named_parameters()})
        losses.append([loss_seg.item(), loss_adv.item(), l_src.item(), l_tgt.item()])
    # NOTE: the discriminator losses above are evaluated before the generator's SGD step, as in the reference (features are
    # detached copies of the pre-update forward), so per-rank losses must match the workers' exactly
    for r in range(2):
        got = np.load(tmp_path / ("fada_losses_%d.npy" % r))
        assert np.allclose(got, losses[r], rtol=1e-5), (r, got, losses[r])
    fe, cls, D = _fada_models()
    lr = 5e-4 * ((1 - 1 / 40) ** 0.9)
    lr_d = 1e-4 * ((1 - 1 / 40) ** 0.9)
    of, oc = ref_model.make_optimizers(fe, cls, 5e-4)
    for g in of.param_groups:
        g["lr"] = lr
    for g in oc.param_groups:
        g["lr"] = lr * 10
    od = torch.optim.Adam(D.parameters(), lr=lr_d, betas=(0.9, 0.99))
    for m in (fe, cls):
        for k, p in m.named_parameters():
            p.grad = (gen_grads[0][k] + gen_grads[1][k]) / 2
    for k, p in D.named_parameters():
        p.grad = (d_grads[0][k] + d_grads[1][k]) / 2
    of.step()
    oc.step()
    od.step()
    want = torch.cat([p.detach().reshape(-1) for m in (fe, cls, D) for p in m.parameters()]).numpy()
    assert np.abs(p0 - want).max() <= 5e-6 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ overlapped exchange
def _overlap_worker(rank, world, port, tmpdir):
    """Stand-in for engine.StageEngine.backward: the real engine reports finished gradient ranges block by block, last block
    first, through FlatStore.grad_hooks (engine.py: `hook(store, lo, hi)` after each bottleneck's weight gradients are enqueued).
    Here autograd produces the gradients and the hooks are fired the same way, so that buckets are exchanged BEFORE finish()."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    try:
        out = {}
        for mode in ("serial", "overlap", "bf16"):
            fe, cls = _models()
            st_cls = engine.FlatStore(list(cls.named_parameters()), torch.device("cpu"))
            st_fe = engine.FlatStore(list(fe.named_parameters()), torch.device("cpu"))
            red = ddp.GradAllReducer([st_cls, st_fe], bucket_bytes=64 << 10, overlap=mode != "serial", payload="bf16" if mode == "bf16" else "fp32")
            assert len(red.buckets[id(st_fe)]) >= 4
            x, lab = _batch(rank)
            torch.nn.functional.cross_entropy(cls(fe(x), lab.shape[-2:]), lab.long(), ignore_index=255).backward()
            local = {"cls": st_cls.grad.clone(), "fe": st_fe.grad.clone()}
            launched_early = 0
            # head first (its gradients complete first), then the backbone's parameters in reverse layout order, four "blocks"
            for hook in st_cls.grad_hooks:
                hook(st_cls, 0, st_cls.total)
            cuts = [st_fe.offsets[i] for i in range(len(st_fe.offsets) - 1, -1, -max(1, len(st_fe.offsets) // 4))] + [0]
            hi = st_fe.total
            for lo in cuts:
                for hook in st_fe.grad_hooks:
                    hook(st_fe, lo, hi)
                hi = lo
                launched_early = sum(b.launched for b in red.buckets[id(st_fe)])
            if mode == "serial":
                assert launched_early == 0                                  # overlap off: nothing leaves before finish()
            else:
                assert launched_early == len(red.buckets[id(st_fe)])        # every bucket was exchanged by a hook, none left for finish()
            red.finish()
            assert not any(b.launched for b in red.buckets[id(st_fe)])      # reset for the next step
            out[mode] = {"cls": st_cls.grad.clone(), "fe": st_fe.grad.clone(), "local": local}
        torch.save(out, os.path.join(tmpdir, "overlap_%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_overlapped_bucket_exchange_and_bf16_payload(tmp_path):
    port = _free_port()
    mp.spawn(_overlap_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / ("overlap_%d.pt" % r)) for r in range(2))
    for tag in ("cls", "fe"):
        want = (r0["serial"]["local"][tag] + r1["serial"]["local"][tag]) / 2
        # fp32 payload: overlapped == serial == the average of the two local gradients, identical on both ranks
        for mode in ("serial", "overlap"):
            assert torch.equal(r0[mode][tag], r1[mode][tag])
            assert torch.allclose(r0[mode][tag], want, rtol=1e-6, atol=1e-12)
        assert torch.equal(r0["serial"][tag], r0["overlap"][tag])
        # bf16 payload: each rank's contribution rounded to bf16, summed in fp32, average rounded to bf16 once
        exp = ((r0["bf16"]["local"][tag].to(torch.bfloat16).float() + r1["bf16"]["local"][tag].to(torch.bfloat16).float()) / 2).to(torch.bfloat16).float()
        assert torch.equal(r0["bf16"][tag], exp) and torch.equal(r1["bf16"][tag], exp)
        err = (r0["bf16"][tag] - want).abs().max() / want.abs().max()
        assert err < 2.0 ** -7, err                                         # two bf16 roundings of an fp32 average


def _bf16_rs_worker(rank, world, port, tmpdir):
    """MI_DDP_PAYLOAD=bf16 as reduce-scatter (all_to_all_single) + all-gather over `world` ranks, bucket sizes that do not divide by it."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    try:
        params = [("p%d" % i, torch.nn.Parameter(torch.zeros(n))) for i, n in enumerate((1000, 67, 5003, 301, 7001, 13))]
        st = engine.FlatStore(params, torch.device("cpu"))
        red = ddp.GradAllReducer([st], bucket_bytes=4 * 3000, payload="bf16")
        assert len(red.buckets[id(st)]) >= 3 and red.diag["ranks"] == world and red.diag["payload"] == "bf16"
        assert red.diag["wire_bytes_per_rank_per_step"] == int(2 * (world - 1) / world * st.total * 2)
        g = torch.Generator().manual_seed(100 + rank)
        for step in range(2):                                    # twice: the per-bucket staging buffers are reused
            local = torch.randn(st.total, generator=g) * (1.0 + step)
            st.grad.copy_(local)
            red.finish()
            torch.save({"local": local, "avg": st.grad.clone()}, os.path.join(tmpdir, "rs_%d_%d.pt" % (step, rank)))
    finally:
        dist.destroy_process_group()


def _check_bf16_rs(tmp_path, world):
    for step in range(2):
        res = [torch.load(tmp_path / ("rs_%d_%d.pt" % (step, r))) for r in range(world)]
        acc = res[0]["local"].to(torch.bfloat16).float()
        for r in range(1, world):
            acc = acc + res[r]["local"].to(torch.bfloat16).float()           # fp32 sum in rank order
        exp = (acc / world).to(torch.bfloat16).float()                        # one rounding of the average
        for r in range(world):
            assert torch.equal(res[r]["avg"], exp), (step, r)


def test_four_rank_gloo_bf16_payload_reduce_scatter_all_gather(tmp_path):
    port = _free_port()
    mp.spawn(_bf16_rs_worker, args=(4, port, str(tmp_path)), nprocs=4, join=True)
    _check_bf16_rs(tmp_path, 4)


def test_two_rank_gloo_bf16_payload_reduce_scatter_all_gather(tmp_path):
    port = _free_port()
    mp.spawn(_bf16_rs_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    _check_bf16_rs(tmp_path, 2)


# ------------------------------------------------------------------------------------------------ synchronised BatchNorm (host logic)
class _TorchBnKernels:
    """Stand-ins for the BatchNorm entry points of kernels.py on CPU tensors (test infrastructure: the product path has no CPU
    kernels) - the same contracts: RAW per-channel sums over NHWC tensors, packed sign bits, fp32 arithmetic."""

    @staticmethod
    def bn_colsum2(y, pilot):
        d = y.float().reshape(-1, y.shape[-1]) - pilot
        return d.sum(0), (d * d).sum(0)

    @staticmethod
    def bn_finalize(s1, s2, pilot, count, bn):
        """mi_bn_finalize's contract: pilot-form sums over `count` pixels -> [mean | invstd | gamma * invstd | beta - mean * gamma * invstd], running
        statistics updated as torch.nn.BatchNorm2d does."""
        d = s1.double() / count
        mean = pilot.double() + d
        var = (s2.double() / count - d * d).clamp_min(0.0)
        invstd = torch.rsqrt(var + bn.eps)
        scale = bn.weight.detach().double() * invstd
        with torch.no_grad():
            m = bn.momentum
            bn.running_mean.copy_(((1 - m) * bn.running_mean.double() + m * mean).float())
            bn.running_var.copy_(((1 - m) * bn.running_var.double() + m * var * count / max(count - 1, 1)).float())
            bn.num_batches_tracked += 1
        return torch.stack([mean, invstd, scale, bn.bias.detach().double() - mean * scale]).float()

    @staticmethod
    def bn_apply(y, mean, scale, beta, res=None, relu=False, want_mask=False):
        out = (y.float() - mean) * scale + beta
        if res is not None:
            out = out + res.float()
        if relu:
            out = out.relu()
        out = out.to(y.dtype)
        return (out, (out.float() > 0)) if want_mask else out

    @staticmethod
    def relu_mask(g, bits):
        return (g.float() * bits).to(g.dtype)

    @staticmethod
    def bn_bwd_colsums(g, y, mean, invstd, relu_bits=None, out=None):
        gf = g.float() * relu_bits if relu_bits is not None else g.float()
        xhat = (y.float() - mean) * invstd
        C = y.shape[-1]
        dbeta, dgamma = gf.reshape(-1, C).sum(0), (gf * xhat).reshape(-1, C).sum(0)
        if out is not None:
            out[0].copy_(dbeta)
            out[1].copy_(dgamma)
            return out
        return dbeta, dgamma

    @staticmethod
    def bn_bwd_apply(g, y, mean, invstd, gamma, dbeta, dgamma, count, relu_bits=None):
        gf = g.float() * relu_bits if relu_bits is not None else g.float()
        xhat = (y.float() - mean) * invstd
        return (gamma * invstd * (gf - dbeta / count - xhat * dgamma / count)).to(g.dtype)


def _syncbn_worker(rank, world, port, tmpdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    try:
        for name in ("bn_colsum2", "bn_finalize", "bn_apply", "relu_mask", "bn_bwd_colsums", "bn_bwd_apply"):
            setattr(engine.K, name, getattr(_TorchBnKernels, name))
        g = torch.Generator().manual_seed(5)
        B, H, W, C = 4, 6, 5, 16
        y_all = torch.randn(B, H, W, C, generator=g) * 1.5 + torch.randn(C, generator=g)
        res_all = torch.randn(B, H, W, C, generator=g)
        gout_all = torch.randn(B, H, W, C, generator=g)

        def run(sl, sync):
            bn = torch.nn.BatchNorm2d(C)
            with torch.no_grad():
                bn.weight.copy_(torch.linspace(0.5, 1.5, C))
                bn.bias.copy_(torch.linspace(-0.2, 0.2, C))
            bn._mi_sync = sync
            # the unit of StageEngine.forward_batchnorm / backward_batchnorm: statistics (+ exchange) -> normalise + residual + ReLU; backward:
            # ReLU mask, affine gradients (this rank's sums), exchange of the sums, input gradient
            y, res = y_all[sl].clone(), res_all[sl].clone()
            fin, count = engine.bn_batch_statistics(y, bn)
            out, bits = engine.K.bn_apply(y, fin[0], fin[2], bn.bias.detach(), res=res, relu=True, want_mask=True)
            dres = engine.K.relu_mask(gout_all[sl], bits)
            dy = engine.bn_backward(dres, y, fin, count, bn)
            return out, dy, dres, bn.weight.grad.clone(), bn.bias.grad.clone(), bn.running_mean.clone(), bn.running_var.clone()

        half = slice(rank * 2, rank * 2 + 2)
        out_s, dy_s, dres_s, dg_s, db_s, rm_s, rv_s = run(half, True)
        dist.all_reduce(dg_s)
        dist.all_reduce(db_s)
        out_f, dy_f, dres_f, dg_f, db_f, rm_f, rv_f = run(slice(0, B), False)
        # torch's own BatchNorm2d on the full batch as the third witness
        bn = torch.nn.BatchNorm2d(C)
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-0.2, 0.2, C))
        yt = y_all.permute(0, 3, 1, 2).clone().requires_grad_(True)
        ot = (bn(yt) + res_all.permute(0, 3, 1, 2)).relu()
        ot.backward(gout_all.permute(0, 3, 1, 2))
        close = lambda a, b, tol=2e-5: float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))
        assert close(out_f, ot.detach().permute(0, 2, 3, 1)) and close(dy_f, yt.grad.permute(0, 2, 3, 1)), "single-process BatchNorm unit vs torch"
        assert close(dg_f, bn.weight.grad) and close(db_f, bn.bias.grad) and close(rm_f, bn.running_mean) and close(rv_f, bn.running_var)
        # synchronised halves == the full batch: outputs, input / residual gradients of this rank's samples, summed affine gradients,
        # running statistics (global mean, unbiased global variance)
        assert close(out_s, out_f[half]) and close(dy_s, dy_f[half]) and close(dres_s, dres_f[half])
        assert close(dg_s, dg_f) and close(db_s, db_f) and close(rm_s, rm_f) and close(rv_s, rv_f)
        # without the exchange the halves differ from the full batch
        out_l = run(half, False)[0]
        assert not close(out_l, out_f[half], 1e-3)
        open(os.path.join(tmpdir, "syncbn_ok_%d" % rank), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_synchronised_batchnorm_equals_full_batch(tmp_path):
    """engine.bn_batch_statistics / bn_backward with `_mi_sync` (train_distill.py:53 SyncBatchNorm semantics) in a 2-rank gloo job, the BatchNorm kernels replaced
    by torch stand-ins with the same contracts: the exchange of RAW sums, the global pixel count, the per-rank affine gradients and
    the running-statistics update reproduce one process on the full batch - and torch.nn.BatchNorm2d itself."""
    port = _free_port()
    mp.spawn(_syncbn_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(os.path.join(str(tmp_path), "syncbn_ok_%d" % r)) for r in range(2))
