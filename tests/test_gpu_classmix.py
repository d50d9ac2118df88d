"""GPU tests of the mean-teacher + ClassMix self-training: the three kernels of csrc/classmix.hip through the wrappers, and whole AsppClassMix
iterations on the tiny depth plan.

Every comparison is exact unless a bound is written at the assert.  The pseudo-labels' oracle is kernels.upsample_predict_score (one source, no
mirror, divisors 1), which has its own parity tests; everything integer is restated in numpy (tests/_classmix_ref.py); the EMA is held against
float64 on the fp32 a and the fp32 b = 1.0f - a with the bound of two rounded products and one rounded sum."""
import logging
import os

import numpy as np
import pytest
import torch

import _classmix_ref as ref
from rnd_semantic_segmentation_amd.host import synth

pytestmark = pytest.mark.gpu

K = None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _kern():
    global K
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from rnd_semantic_segmentation_amd import kernels
    K = kernels
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ mi_label_classes
def label_case(H, W, nc, seed):
    """B = 3: an all-ignore image, a one-class image, and an image of every class but one - which occurs in the single last pixel - with ignore and
    out-of-range values sprinkled in."""
    rng = np.random.RandomState(seed)
    lab = np.full((3, H, W), 255, dtype=np.int64)
    lab[1] = nc - 1
    lone = nc // 2
    pool = np.array([c for c in range(nc) if c != lone] + [255, nc, -1, 300, 2 ** 40, -2 ** 40], dtype=np.int64)
    lab[2] = pool[rng.randint(0, len(pool), size=(H, W))]
    lab[2, H - 1, W - 1] = lone
    return lab


# 33 x 49 and 129 x 257: odd planes (one label per load); 34 x 50: an even plane, two labels per load
@pytest.mark.parametrize("nc", [19, 32])
@pytest.mark.parametrize("H,W", [(33, 49), (129, 257), (34, 50)])
def test_label_classes_matches_numpy(H, W, nc):
    lab = label_case(H, W, nc, seed=H + nc)
    want = ref.present_bits(lab, nc)
    assert want[0] == 0 and want[1] == np.uint32(1) << np.uint32(nc - 1) and want[2] == np.uint32((1 << nc) - 1)      # the lone last pixel counts
    dirty = torch.full((3,), -1, dtype=torch.int32, device="cuda")          # the entry zeroes what it is given
    got = K.label_classes(dev(lab), nc, out=dirty)
    assert got is dirty and np.array_equal(bits(got), want)
    assert np.array_equal(bits(K.label_classes(dev(lab), nc)), want)
    if nc == 32:                                            # the same labels under K = 19: classes 19..31 are out of range now
        assert np.array_equal(bits(K.label_classes(dev(lab), 19)), ref.present_bits(lab, 19))


# ------------------------------------------------------------------------------------------------ mi_classmix
IGNORE = 255


def mix_case(h, w, H, W, nc, seed, B=2):
    """Teacher logits whose scale ramps from 0.25 to 48 across the low-resolution columns (max probability from near 1/K up to a rounded 1.0),
    source labels in blocks of 8 x 8 with ignore / out-of-range values, and two unrelated images."""
    rng = np.random.RandomState(seed)
    low = rng.randn(B, h, w, nc).astype(np.float32) * np.linspace(0.25, 48.0, w, dtype=np.float32)[None, None, :, None]
    pool = np.array(list(range(nc)) + [IGNORE, nc, -1], dtype=np.int64)
    blocks = pool[rng.randint(0, len(pool), size=(B, (H + 7) // 8, (W + 7) // 8))]
    lab = np.repeat(np.repeat(blocks, 8, 1), 8, 2)[:, :H, :W].copy()
    src = rng.randn(B, 3, H, W).astype(np.float32)
    tgt = rng.randn(B, 3, H, W).astype(np.float32)
    prio = np.stack([rng.permutation(nc) for _ in range(B)]).astype(np.uint8)
    return dict(low=low, lab=lab, src=src, tgt=tgt, prio=prio, nc=nc, size=(H, W))


def oracle_pseudo(low_dev, size, t):
    return np.stack([K.upsample_predict_score([low_dev[b]], [False], size, 1.0, 1.0, threshold=t, want_pseudo=True)[1].cpu().numpy()
                     for b in range(low_dev.shape[0])])


def run_mix(c, t, want_mask=True, out_img=None, ignore=IGNORE):
    low, lab = dev(c["low"]), dev(c["lab"])
    present = K.label_classes(lab, c["nc"])
    r = K.classmix(dev(c["src"]), dev(c["tgt"]), lab, low, present, dev(c["prio"]), t, ignore, out_img=out_img, want_mask=want_mask)
    pseudo = oracle_pseudo(low, c["size"], t)
    want = ref.classmix(c["src"], c["tgt"], c["lab"], pseudo, ref.present_bits(c["lab"], c["nc"]), c["prio"], c["nc"], ignore)
    return r, want, pseudo


# 5 x 7 -> 33 x 49 (K = 19 and K = 2), 17 x 33 -> 129 x 257 (several workgroups per image, rows that straddle them); 5 x 7 -> 34 x 50: even rows,
# two pixels per lane
@pytest.mark.parametrize("t", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("h,w,H,W,nc", [(5, 7, 33, 49, 19), (5, 7, 33, 49, 2), (17, 33, 129, 257, 19), (5, 7, 34, 50, 19)])
def test_classmix_matches_oracle_and_restatement(h, w, H, W, nc, t):
    c = mix_case(h, w, H, W, nc, seed=H + nc)
    r, (img, lab, mask, counts), pseudo = run_mix(c, t)
    got_mask = r.mask.cpu().numpy()
    assert np.array_equal(got_mask, mask) and 0 < int(mask.sum()) < mask.size
    out = mask == 0
    ignored = int((pseudo[out] == 255).sum())
    print("classmix %dx%d K=%d t=%.1f: pasted %d, unpasted kept %d, ignored %d" % (H, W, nc, t, mask.sum(), counts[:, 1].sum(), ignored))
    if t == 1.0 or (t == 0.5 and nc > 2):                   # (t = 0 keeps every pixel; with two classes the maximum is never below 0.5)
        assert 0 < ignored < int(out.sum())                 # a mixed kept / ignored picture
    else:
        assert ignored == 0
    got_lab = r.label.cpu().numpy()
    want_outside = np.where(pseudo == 255, IGNORE, pseudo.astype(np.int64))
    assert np.array_equal(got_lab[out], want_outside[out])                   # bit for bit the evaluation tail's pseudo-labels, no pixel left out
    assert np.array_equal(got_lab, lab)                                      # ... and the source labels inside the mask
    assert np.array_equal(r.image.cpu().numpy().view(np.uint32), img.view(np.uint32))
    assert np.array_equal(r.counts.cpu().numpy(), counts)


def test_classmix_empty_and_full_selection():
    c = mix_case(5, 7, 33, 49, 19, seed=5)
    c["lab"][0] = IGNORE                                    # nothing present: chosen is empty, the mixed image is the target image
    c["lab"][1] = 7                                         # one class: it is chosen, the whole image is pasted
    r, (img, lab, mask, counts), pseudo = run_mix(c, 0.5)
    assert mask[0].sum() == 0 and mask[1].all() and counts[0, 0] == 0 and counts[1].tolist() == [33 * 49, 0]
    assert np.array_equal(r.mask.cpu().numpy(), mask) and np.array_equal(r.counts.cpu().numpy(), counts)
    assert np.array_equal(r.label.cpu().numpy(), lab) and np.array_equal(r.image.cpu().numpy(), img)
    assert np.array_equal(r.image[0].cpu().numpy(), c["tgt"][0]) and np.array_equal(r.image[1].cpu().numpy(), c["src"][1])
    assert (r.label[1] == 7).all()


def test_classmix_without_mask_in_a_slice_of_a_larger_buffer_twice():
    c = mix_case(17, 33, 129, 257, 19, seed=9)
    B, (H, W) = 2, c["size"]
    big = torch.full((2 * B, 3, H, W), 7.0, device="cuda")
    r, (img, lab, mask, counts), _ = run_mix(c, 0.5, want_mask=False, out_img=big[B:], ignore=-1)
    assert r.mask is None and r.image.data_ptr() == big[B:].data_ptr()
    assert np.array_equal(big[B:].cpu().numpy(), img) and (big[:B] == 7.0).all()          # the first half is not touched
    assert np.array_equal(r.label.cpu().numpy(), lab) and (lab == -1).any()
    assert np.array_equal(r.counts.cpu().numpy(), counts)
    again, _, _ = run_mix(c, 0.5, want_mask=False, ignore=-1)                              # two runs are bit-equal
    assert torch.equal(again.image.view(torch.int32), r.image.view(torch.int32)) and torch.equal(again.label, r.label)
    assert torch.equal(again.counts, r.counts)


def test_classmix_zeroes_a_dirty_counts_buffer():
    from rnd_semantic_segmentation_amd import _lib
    c = mix_case(5, 7, 33, 49, 19, seed=11)
    H, W = c["size"]
    low, lab, src, tgt, prio = dev(c["low"]), dev(c["lab"]), dev(c["src"]), dev(c["tgt"]), dev(c["prio"])
    present = K.label_classes(lab, 19)
    img, out = torch.empty_like(src), torch.empty_like(lab)
    counts = torch.full((2, 2), 12345, dtype=torch.int64, device="cuda")
    p = K._p
    _lib.check(_lib.lib().mi_classmix(p(src), p(tgt), p(lab), p(low), p(present), p(prio), 0.5, IGNORE, p(img), p(out), None, p(counts), 2, 5, 7, 19,
                                      H, W, K._stream()), "mi_classmix")
    clean = K.classmix(src, tgt, lab, low, present, prio, 0.5, IGNORE)
    assert torch.equal(counts, clean.counts) and torch.equal(out, clean.label) and int(counts.sum()) > 0


# ------------------------------------------------------------------------------------------------ mi_ema_update
PAD = 8


@pytest.mark.parametrize("a", [0.0, 0.5, 0.99, 1.0])
@pytest.mark.parametrize("n", [1, 7, 4099, 2 ** 20 + 3])
def test_ema_update_against_float64(n, a):
    rng = np.random.RandomState(n % 1000)
    hyper = torch.tensor([a], dtype=torch.float32, device="cuda")
    for off_t, off_s in ((0, 0), (1, 1), (1, 0), (0, 1), (3, 2)):          # floats past a 16-byte boundary
        t0 = rng.randn(PAD + off_t + n + PAD).astype(np.float32)
        s0 = rng.randn(PAD + off_s + n + PAD).astype(np.float32)
        tb, sb = dev(t0), dev(s0)
        lo_t, lo_s = PAD + off_t, PAD + off_s
        assert tb.data_ptr() % 16 == 0 and sb.data_ptr() % 16 == 0
        K.ema_update(tb[lo_t:lo_t + n], sb[lo_s:lo_s + n], hyper)
        got = tb.cpu().numpy()
        exact, bound = ref.ema_exact(t0[lo_t:lo_t + n], s0[lo_s:lo_s + n], a)
        err = np.abs(got[lo_t:lo_t + n].astype(np.float64) - exact)
        assert (err <= bound).all(), (off_t, off_s, float((err - bound).max()))      # 3 * 2**-24 * (|a t| + |b s|)
        if a == 0.0:
            assert np.array_equal(got[lo_t:lo_t + n], s0[lo_s:lo_s + n])
        if a == 1.0:
            assert np.array_equal(got[lo_t:lo_t + n], t0[lo_t:lo_t + n])
        assert np.array_equal(got[:lo_t], t0[:lo_t]) and np.array_equal(got[lo_t + n:], t0[lo_t + n:])      # nothing outside the range is touched
        assert np.array_equal(sb.cpu().numpy(), s0)


# ------------------------------------------------------------------------------------------------ whole iterations
HEAD_SCALE = 64.0          # formula weights leave the head's probabilities within 0.06 .. 0.065; a head 64 x as large spreads them over 0.45 .. 1
THRESH = 0.8               # ... so that this threshold keeps about half of the target pixels


def mix_inputs():
    xs, ys = synth.synth_image(2, 65, 97, seed=71), synth.synth_label(2, 65, 97, 19, seed=71)
    xt = synth.synth_image(2, 65, 97, seed=72)
    return torch.from_numpy(xs), torch.from_numpy(ys), torch.from_numpy(xt)


def _builders(monkeypatch, layers=(1, 1, 2, 2)):
    from rnd_semantic_segmentation_amd.host import modules
    from rnd_semantic_segmentation_amd.host import trainer as tr

    def backbone(cfg):
        m = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False, layers=layers)
        synth.load_formula_weights(m)
        return m

    def head(cfg):
        m = modules.build_classifier(cfg)
        synth.load_formula_weights(m)
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(HEAD_SCALE)
        return m

    monkeypatch.setattr(tr.ASPPTrainer, "build_feature_extractor", staticmethod(backbone))
    monkeypatch.setattr(tr.ASPPTrainer, "build_classifier", staticmethod(head))
    return backbone, head


def _combo(tmp_path, monkeypatch, fused=True, resume=""):
    """AsppClassMix on the product modules (tiny depth plan, formula weights), as tests/test_gpu_fada.py builds AsppFada."""
    from rnd_semantic_segmentation_amd.host import config as hc
    from rnd_semantic_segmentation_amd.host import self_train
    cfg = hc.CfgNode(hc.default_tree())
    cfg.merge_from_file(os.path.join(ROOT, "configs", "deeplabv2_r101_classmix.yaml"))
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path), "SOLVER.BASE_LR", 5e-4, "SOLVER.MIX_THRESHOLD", THRESH, "resume", resume])
    cfg.freeze()
    _builders(monkeypatch)
    monkeypatch.setattr(self_train, "setup_logger", lambda *a, **k: logging.getLogger("test_gpu_classmix"))
    combo = self_train.AsppClassMix("aspp_classmix", cfg, [], [], 0)
    combo.FUSED, combo.KEEP_MIX = fused, True
    return combo


def _params(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_one_iteration_fused_against_literal(tmp_path, monkeypatch):
    xs, ys, xt = mix_inputs()
    got = {}
    for fused in (True, False):
        combo = _combo(tmp_path, monkeypatch, fused=fused)
        combo.iteration = 5                                 # a = 1 - 1/6: the update mixes (iteration 0 only copies the student)
        before = [_params(combo.teacher_feature_extractor), _params(combo.teacher_classifier)]
        r = combo.train_step(xs, ys, xt, 40)
        torch.cuda.synchronize()
        got[fused] = dict(img=combo.last_mix[0].clone(), lab=combo.last_mix[1].clone(), loss=r["loss"].clone(), counts=r["counts"].clone(),
                          student=[_params(combo.aspp.feature_extractor), _params(combo.aspp.classifier)], before=before,
                          pnames=[{n for n, _ in m.named_parameters()} for m in (combo.teacher_feature_extractor, combo.teacher_classifier)],
                          teacher=[_params(combo.teacher_feature_extractor), _params(combo.teacher_classifier)])
    f, l = got[True], got[False]
    px = 2 * 65 * 97
    pasted, kept = (int(v) for v in f["counts"].sum(0))
    print("combo: pasted %d, kept %d of %d unpasted, loss %.6f" % (pasted, kept, px - pasted, float(f["loss"])))
    assert 0 < pasted < px and 0 < kept < px - pasted                        # the inputs exercise both branches of both selections
    assert torch.equal(f["img"].view(torch.int32), l["img"].view(torch.int32)) and torch.equal(f["lab"], l["lab"])
    assert torch.equal(f["counts"], l["counts"])
    assert torch.equal(f["loss"], l["loss"]) and np.isfinite(float(f["loss"]))
    for i in range(2):
        assert _same(f["student"][i], l["student"][i])
    a = 1.0 - 1.0 / 6.0
    for g in (f, l):                                        # either path's teacher lies within the EMA bound of the exact update
        for i in range(2):
            for k, t0 in g["before"][i].items():
                if k not in g["pnames"][i]:
                    assert torch.equal(g["teacher"][i][k], t0), k            # FrozenBatchNorm buffers do not move
                    continue
                exact, bound = ref.ema_exact(t0.cpu().numpy(), g["student"][i][k].cpu().numpy(), a)
                assert (np.abs(g["teacher"][i][k].cpu().numpy().astype(np.float64) - exact) <= bound).all(), k


def test_teacher_is_repacked_after_the_update(tmp_path, monkeypatch):
    xs, ys, xt = mix_inputs()
    combo = _combo(tmp_path, monkeypatch)
    combo.iteration = 3
    combo.train_step(xs, ys, xt, 40)
    low = combo._teacher_low(xt.cuda())
    backbone, head = _builders(monkeypatch)
    fe, cls = backbone(None).cuda().eval(), head(combo.cfg).cuda().eval()
    fe.load_state_dict(combo.teacher_feature_extractor.state_dict())
    cls.load_state_dict(combo.teacher_classifier.state_dict())
    with torch.no_grad():
        fresh = cls(fe(xt.cuda())).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(low, fresh)
    with torch.no_grad():                                   # ... and they are not the student's
        student = combo.aspp.classifier(combo.aspp.feature_extractor(xt.cuda())).permute(0, 2, 3, 1)
    assert not torch.equal(low, student)


def test_three_iterations_are_finite_and_reproducible(tmp_path, monkeypatch):
    xs, ys, xt = mix_inputs()
    runs = []
    for _ in range(2):
        combo = _combo(tmp_path, monkeypatch)
        losses = [combo.train_step(xs, ys, xt, 40)["loss"] for _ in range(3)]
        runs.append(([float(v) for v in losses], _params(combo.teacher_classifier), _params(combo.aspp.classifier),
                     _params(combo.teacher_feature_extractor)))
    assert all(np.isfinite(runs[0][0])) and combo.iteration == 3
    assert runs[0][0] == runs[1][0] and _same(runs[0][1], runs[1][1]) and _same(runs[0][2], runs[1][2]) and _same(runs[0][3], runs[1][3])
    assert not _same(runs[0][1], runs[0][2])                # teacher != student after three updates (a = 0, 1/2, 2/3)


def test_checkpoint_round_trip(tmp_path, monkeypatch):
    from rnd_semantic_segmentation_amd.host import tester
    xs, ys, xt = mix_inputs()
    combo = _combo(tmp_path, monkeypatch)
    for _ in range(2):
        combo.train_step(xs, ys, xt, 40)
    path = str(tmp_path / "AsppClassMix-1.pth")
    combo._save_checkpoint(1, path)
    student = [_params(combo.aspp.feature_extractor), _params(combo.aspp.classifier)]
    teacher = [_params(combo.teacher_feature_extractor), _params(combo.teacher_classifier)]
    # test.py's loading path evaluates the student unchanged
    backbone, head = _builders(monkeypatch)
    monkeypatch.setattr(tester.ASPPTester, "build_feature_extractor", staticmethod(backbone))
    monkeypatch.setattr(tester.ASPPTester, "build_classifier", staticmethod(head))
    cfg = combo.cfg.clone()
    cfg.defrost()
    cfg.merge_from_list(["resume", path])
    t = tester.ASPPTester(cfg, torch.device("cuda"), [], logging.getLogger("test_gpu_classmix"), None, None)
    t._load_checkpoint()
    assert _same(_params(t.feature_extractor), student[0]) and _same(_params(t.classifier), student[1])
    # the combo resumes with both nets and the position restored
    again = _combo(tmp_path, monkeypatch, resume=path)
    assert again.iteration == 2 and again.start_epoch == 2
    assert _same(_params(again.aspp.feature_extractor), student[0]) and _same(_params(again.aspp.classifier), student[1])
    assert _same(_params(again.teacher_feature_extractor), teacher[0]) and _same(_params(again.teacher_classifier), teacher[1])
    assert not _same(teacher[1], student[1])
    r = again.train_step(xs, ys, xt, 40)                    # ... and goes on
    assert np.isfinite(float(r["loss"])) and again.iteration == 3
