"""mi_sgd_step_pack / mi_sgd_step_pack_dev (csrc/elementwise.hip): the SGD update of a whole flat store and the bf16 repack of its conv weights in one
launch, against the two launches it replaces.  Bit for bit (torch.equal on integer views): p and buf are mi_sgd_step's on a copy, wp / wpt are what
mi_pack_weights_multi writes from that updated copy.

Kernel level: a flat buffer of 200 003 floats - an uncovered 9 408-float span at the front (the stem weight's place), table rows (O, I, T) = (64, 64, 1),
(64, 64, 9), (32, 160, 1), (40, 72, 9) (a second o tile of 8 rows, a second i group, a last i tile of 8 columns), a second uncovered span between the rows
and a 3-float tail, which mi_sgd_step updates with its differently contracted tail code; one row without a data-gradient pack (wpt_off = -1), one without
a folded scale (scale_off = -1).  Two consecutive steps, by-value and device hyper-parameters.  A second table holds shapes that keep no 16-byte access
aligned (odd offsets, I = 70 and 36, O = 20), which the old pack accepts and the new launch must too.
Engine level: ASPPTrainer steps at 2 x 65 x 65 with MI_SGD_PACK on and off: parameters, momentum and both packed buffers equal after each step, no
mi_pack_weights_multi in a steady-state step with it on, and one again after an eval() forward in between."""
import logging

import pytest
import torch

import _cases
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, MU, WD = 2.5e-4, 0.9, 5e-4


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rnd_semantic_segmentation_amd import kernels
    return kernels


def _layout(shapes, front, mid, tail, odd=0):
    """rows [w_off, scale_off, wp_off, wpt_off, O, I, T, first_block] laid out behind `front` uncovered floats, `mid` more after the second row,
    `tail` at the end; odd: extra floats in front of every row (unaligned offsets)."""
    rows, off, soff, poff, blk = [], front, 0, 0, 0
    for k, (O, I, T) in enumerate(shapes):
        off += odd
        poff += odd
        rows.append([off, soff, poff, poff, O, I, T, blk])
        off += O * I * T
        poff += O * I * T
        soff += O
        blk += -(-O // 32) * -(-I // 128)
        if k == 1:
            off += mid
    return rows, off + tail, soff, poff, blk


def _run(K, rows, n, n_scale, n_pack, blocks, dev_hyper):
    g = torch.Generator(device="cpu").manual_seed(n)
    p = torch.randn(n, generator=g).to(DEV)
    buf = torch.randn(n, generator=g).to(DEV)
    sflat = (torch.rand(n_scale, generator=g) + 0.5).to(DEV)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    gaps = K.pack_table_gaps(rows, n)
    gaps_dev = torch.tensor(gaps, dtype=torch.int64, device=DEV) if gaps else None
    hyper = torch.tensor([LR, MU, WD], dtype=torch.float32, device=DEV)
    wp = torch.full((n_pack,), 7.0, dtype=torch.bfloat16, device=DEV)
    wpt = torch.full((n_pack,), 7.0, dtype=torch.bfloat16, device=DEV)
    p_ref, buf_ref, wp_ref, wpt_ref = p.clone(), buf.clone(), wp.clone(), wpt.clone()
    for step in range(2):
        grad = torch.randn(n, generator=g).to(DEV)
        K.sgd_step_pack(p, grad, buf, hyper if dev_hyper else LR, MU, WD, sflat, wp, wpt, table, len(rows), blocks, gaps_dev)
        if dev_hyper:
            K.sgd_step_dev(p_ref, grad, buf_ref, hyper)
        else:
            K.sgd_step(p_ref, grad, buf_ref, LR, MU, WD)
        K.pack_weights_multi(p_ref, sflat, wp_ref, wpt_ref, table, len(rows), blocks)
        assert torch.equal(p.view(torch.int32), p_ref.view(torch.int32)), step
        assert torch.equal(buf.view(torch.int32), buf_ref.view(torch.int32)), step
        assert torch.equal(wp.view(torch.int16), wp_ref.view(torch.int16)), step
        assert torch.equal(wpt.view(torch.int16), wpt_ref.view(torch.int16)), step
    assert bool((wp != 7.0).any()) and bool((wpt != 7.0).any()) and bool((wpt == 7.0).any())


@pytest.mark.parametrize("dev_hyper", [False, True])
def test_fused_step_has_the_bits_of_sgd_step_plus_pack(K, dev_hyper):
    rows, n, n_scale, n_pack, blocks = _layout([(64, 64, 1), (64, 64, 9), (32, 160, 1), (40, 72, 9)], 9408, 118592, 3)
    assert n == 200003 and n % 4 == 3
    rows[1][3] = -1            # no data-gradient pack
    rows[2][1] = -1            # no folded scale
    assert K.pack_table_gaps(rows, n) == [[0, 9408], [9408 + 4096 + 36864, 9408 + 4096 + 36864 + 118592], [n - 3, n]]
    _run(K, rows, n, n_scale, n_pack, blocks, dev_hyper)


@pytest.mark.parametrize("dev_hyper", [False, True])
def test_shapes_without_16_byte_alignment_are_accepted(K, dev_hyper):
    rows, n, n_scale, n_pack, blocks = _layout([(20, 70, 9), (24, 36, 1), (33, 130, 1)], 5, 7, 2, odd=1)
    rows[2][3] = -1
    _run(K, rows, n, n_scale, n_pack, blocks, dev_hyper)


def test_engine_steps_with_the_switch_on_and_off(K, tmp_path, monkeypatch):
    from rnd_semantic_segmentation_amd.host import config as hc
    from rnd_semantic_segmentation_amd.host.trainer import ASPPTrainer
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_list(["MODEL.FREEZE_BN", True, "MODEL.NUM_CLASSES", 19, "SOLVER.BASE_LR", 5e-4, "OUTPUT_DIR", str(tmp_path)])
    cfg.freeze()
    tr = ASPPTrainer("aspp", cfg, [None] * 50, 0, logger=logging.getLogger("sgd-pack"))
    fe, cls = tr.feature_extractor, tr.classifier
    with torch.no_grad():
        for m in (fe, cls):
            synth.load_formula_weights(m)
            m._store.generation += 1
    fe.train()
    cls.train()
    snap = [m._store.data.clone() for m in (fe, cls)]
    x, lab = _cases.net_inputs(2, 65, 37)
    xt, lt = torch.from_numpy(x), torch.from_numpy(lab)
    packs, real = [], K.pack_weights_multi
    monkeypatch.setattr(K, "pack_weights_multi", lambda *a, **k: (packs.append(1), real(*a, **k))[1])
    eng = fe._engine

    def state():
        n = len(packs)
        eng.prepare(True)                  # switch off: the packs of the new weights are made here; on: they stand already
        made = len(packs) - n
        torch.cuda.synchronize()
        mom = [f.clone() for opt in (tr.optimizer_fea, tr.optimizer_cls) for f in opt._flat_mom.values()]
        return [m._store.data.clone() for m in (fe, cls)] + mom + [eng._wp_flat.clone(), eng._wpt_flat.clone()], made

    out = {}
    for on in (True, False):
        monkeypatch.setattr(K, "sgd_pack_enabled", lambda on=on: on)
        with torch.no_grad():
            for m, s in zip((fe, cls), snap):
                m._store.data.copy_(s)
                m._store.generation += 1
            for opt in (tr.optimizer_fea, tr.optimizer_cls):
                for f in opt._flat_mom.values():
                    f.zero_()
        tr.iteration = 0
        states, counts = [], []
        for step in range(3):
            del packs[:]
            if step == 2:                  # an evaluation between two training steps
                fe.eval()
                with torch.no_grad():
                    fe(xt.to(DEV))
                    fe(xt.to(DEV))
                fe.train()
            in_eval = len(packs)
            tr.train_step(xt, lt, 40)
            in_step = len(packs) - in_eval
            st, made = state()
            states.append(st)
            counts.append((in_eval, in_step, made))
            tr.iteration += 1
        out[on] = (states, counts)
    # (packs in the evaluation, in the training step, in state()).  On: the first step packs once (new weights were loaded), the second not at all; the
    # first eval() forward after a fused step goes back to mi_pack_weights_multi, the second finds those packs, and so does the step after it
    assert out[True][1] == [(0, 1, 0), (0, 0, 0), (1, 0, 0)], out[True][1]
    # off: every update leaves stale packs, which the next prepare() (here: the one in state()) renews; the first step also packs the loaded weights
    assert out[False][1] == [(0, 1, 1), (0, 0, 1), (0, 0, 1)], out[False][1]
    for step, (a, b) in enumerate(zip(out[True][0], out[False][0])):
        assert len(a) == len(b) == 6
        for u, v in zip(a, b):
            assert float(u.float().abs().max()) > 0
            assert torch.equal(u.view(torch.int16), v.view(torch.int16)), step
