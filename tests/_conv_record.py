"""One eager training step of each bench workload that runs on the implicit-GEMM conv family (csrc/igemm_nt.hip, igemm_pp.hip, igemm_tn.hip), built the
way bench.py builds them, with kernels.ROUTES recording: the plan names behind tests/_conv_cases.py PRODUCTION.  GPU only."""
import logging
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(routes):
    return {r.name for r in routes}


def _record(K, step):
    K.ROUTES = set()
    try:
        step()
        torch.cuda.synchronize()
        return _names(K.ROUTES)
    finally:
        K.ROUTES = None


def _deeplab(K, freeze_bn, out_dir, batch=8, size=769):
    """bench.py main(): --workload deeplab (freeze_bn) / deeplab_bn"""
    from bench import synthetic_batch
    from rnd_semantic_segmentation_amd.host import config as hc, synth
    from rnd_semantic_segmentation_amd.host.trainer import ASPPTrainer
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_src.yaml"))
    cfg.merge_from_list(["OUTPUT_DIR", out_dir])
    if not freeze_bn:
        cfg.merge_from_list(["MODEL.FREEZE_BN", "False"])
    cfg.freeze()
    log = logging.getLogger("conv_record")
    log.addHandler(logging.NullHandler())
    trainer = ASPPTrainer("aspp", cfg, [None] * 1000, 0, logger=log)
    with torch.no_grad():
        for m in (trainer.feature_extractor, trainer.classifier):
            synth.load_formula_weights(m)
            st = getattr(m, "_store", None)
            if st is not None:
                st.generation += 1
    x, lab = synthetic_batch(batch, size, 0, torch.device("cuda", 0))
    return _record(K, lambda: trainer.train_step(x, lab, 100000))


def _fada(K, out_dir, batch=8, size=769):
    """bench.py aux_workload(): --workload fada"""
    from rnd_semantic_segmentation_amd.host import config as hc, fada, modules, synth
    from rnd_semantic_segmentation_amd.host import trainer as tr
    dev = torch.device("cuda", 0)
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_adv.yaml"))
    cfg.merge_from_list(["OUTPUT_DIR", out_dir])
    cfg.freeze()

    def formula(m):
        synth.load_formula_weights(m)
        return m
    saved = (tr.ASPPTrainer.__dict__["build_feature_extractor"], tr.ASPPTrainer.__dict__["build_classifier"],
             fada.FADAAdapter.__dict__["build_adversarial_discriminator"], fada.setup_logger)
    b_fe, b_cls, b_d = modules.build_feature_extractor, modules.build_classifier, fada.build_adversarial_discriminator
    try:
        tr.ASPPTrainer.build_feature_extractor = staticmethod(lambda c: formula(b_fe(c)))
        tr.ASPPTrainer.build_classifier = staticmethod(lambda c: formula(b_cls(c)))
        fada.FADAAdapter.build_adversarial_discriminator = staticmethod(lambda c: formula(b_d(c)))
        fada.setup_logger = lambda *a, **k: logging.getLogger("conv_record_fada")
        combo = fada.AsppFada("aspp_fada", cfg, [], [], 0)
    finally:
        tr.ASPPTrainer.build_feature_extractor, tr.ASPPTrainer.build_classifier = saved[0], saved[1]
        fada.FADAAdapter.build_adversarial_discriminator, fada.setup_logger = saved[2], saved[3]
    hb = batch // 2
    xs = torch.from_numpy(synth.synth_image(hb, size, size, seed=1)).to(dev)
    ys = torch.from_numpy(synth.synth_label(hb, size, size, 19, seed=1)).to(dev)
    xt = torch.from_numpy(synth.synth_image(hb, size, size, seed=2)).to(dev)
    return _record(K, lambda: combo.train_step(xs, ys, xt, 10000))


def record_production(K, out_dir):
    """{workload: set of plan names} of one eager step of bench.py's default, deeplab_bn and fada workloads (B = 8, 769 x 769)."""
    seen = {}
    for wl, run in (("deeplab", lambda: _deeplab(K, True, out_dir)), ("deeplab_bn", lambda: _deeplab(K, False, out_dir)), ("fada", lambda: _fada(K, out_dir))):
        seen[wl] = run()
        torch.cuda.empty_cache()
    return seen
