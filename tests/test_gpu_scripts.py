"""Drop-in scripts on the GPU: `train_src.py` (reference flags) trains DeepLabV2-R101 for a few iterations on synthetic
crops, writes Aspp-1.pth + aspp_chart_params.json; `test.py` resumes from it and writes aspp_confusion_matrix.json; `train_adv.py` continues from it with the FADA adversarial step."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args, env_extra):
    env = dict(os.environ, **env_extra)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def test_train_src_then_test_py_roundtrip(tmp_path):
    out = str(tmp_path / "run")
    # an un-pretrained ResNet-101 with identity FrozenBN diverges at once (loss 1.7e5 then NaN in the reference
    # too), so the backbone is initialised the way the reference does it: MODEL.WEIGHTS -> a (local) checkpoint file
    from rnd_semantic_segmentation_amd.host import modules, synth
    fe = modules.resnet_feature_extractor("resnet101", freeze_bn=True, pretrained_backbone=False)
    weights = str(tmp_path / "r101_formula.pth")
    torch.save({k: torch.from_numpy(synth.formula_tensor("backbone." + k, v.shape)) for k, v in fe.backbone.state_dict().items()}, weights)
    r = run(["train_src.py", "-cfg", "configs/deeplabv2_r101_src.yaml", "OUTPUT_DIR", out, "SOLVER.EPOCHS", "1", "MODEL.WEIGHTS", weights,
             "SOLVER.BATCH_SIZE", "2", "INPUT.SOURCE_INPUT_SIZE_TRAIN", "(161, 129)"], {"MI_SYNTH_LEN": "6"})
    assert r.returncode == 0, r.stderr[-3000:]
    chart = json.load(open(os.path.join(out, "aspp_chart_params.json")))
    assert len(chart["loss"]) == 3 and all(0 < v < 10 for v in chart["loss"]) and len(chart["learning rate"]) == 3
    ck = torch.load(os.path.join(out, "Aspp-1.pth"), map_location="cpu")
    assert ck["epoch"] == 1 and ck["iteration"] == 3
    assert len(ck["feature_extractor"]) == 520 and len(ck["classifier"]) == 8
    assert "momentum_buffer" in ck["optimizer_fea"]["state"][0]
    r = run(["test.py", "-cfg", "configs/deeplabv2_r101_src.yaml", "OUTPUT_DIR", out, "resume", os.path.join(out, "Aspp-1.pth"),
             "INPUT.INPUT_SIZE_TEST", "(193, 97)"], {"MI_SYNTH_LEN": "2"})
    assert r.returncode == 0, r.stderr[-3000:]
    cm = json.load(open(os.path.join(out, "aspp_confusion_matrix.json")))
    assert len(cm["cmt"]) == 19 and cm["classes"][0] == "road" and sum(map(sum, cm["cmt"])) > 0
    assert "Micro metric, val result: mIoU/mF1" in r.stderr + r.stdout
    # train_adv.py (FADA) resumes from the source-only checkpoint, as the reference's workflow does; run as a single-rank RCCL job
    # with MI_DDP_FORCE=1 so that the generator-side and discriminator-side gradient reducers issue their collectives
    adv = str(tmp_path / "adv")
    r = run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29541",
             "train_adv.py", "-cfg", "configs/deeplabv2_r101_adv.yaml", "OUTPUT_DIR", adv, "SOLVER.EPOCHS", "1", "MODEL.WEIGHTS", weights,
             "resume", os.path.join(out, "Aspp-1.pth"), "SOLVER.BATCH_SIZE", "4", "INPUT.SOURCE_INPUT_SIZE_TRAIN", "(161, 129)",
             "INPUT.TARGET_INPUT_SIZE_TRAIN", "(129, 129)"], {"MI_SYNTH_LEN": "6", "MI_DDP_FORCE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    chart = json.load(open(os.path.join(adv, "aspp_fada_chart_params.json")))
    assert len(chart["segmentation loss"]) == 3 and all(0 < v < 10 for v in chart["segmentation loss"])
    assert all(0 < v < 10 for v in chart["source discriminator loss"] + chart["target discriminator loss"])
    ck = torch.load(os.path.join(adv, "AsppFada-1.pth"), map_location="cpu")
    assert ck["adv_epoch"] == 1 and ck["iteration"] == 3 and len(ck["model_D"]) == 8
    assert set(ck["optimizer_D"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_train_src_with_trainable_batchnorm_then_test_py(tmp_path):
    """MODEL.FREEZE_BN False through the unchanged scripts: nn.BatchNorm2d backbone (624 state keys), batch statistics while training,
    running statistics in test.py; the optimizer state covers the 312 backbone tensors."""
    out = str(tmp_path / "run_bn")
    r = run(["train_src.py", "-cfg", "configs/deeplabv2_r101_src.yaml", "OUTPUT_DIR", out, "SOLVER.EPOCHS", "1", "MODEL.FREEZE_BN", "False",
             "SOLVER.BATCH_SIZE", "2", "INPUT.SOURCE_INPUT_SIZE_TRAIN", "(161, 129)"], {"MI_SYNTH_LEN": "6"})
    assert r.returncode == 0, r.stderr[-3000:]
    chart = json.load(open(os.path.join(out, "aspp_chart_params.json")))
    assert len(chart["loss"]) == 3 and all(0 < v < 10 for v in chart["loss"])
    ck = torch.load(os.path.join(out, "Aspp-1.pth"), map_location="cpu")
    assert len(ck["feature_extractor"]) == 624 and int(ck["feature_extractor"]["backbone.bn1.num_batches_tracked"]) == 3
    assert len(ck["optimizer_fea"]["state"]) == 312
    r = run(["test.py", "-cfg", "configs/deeplabv2_r101_src.yaml", "OUTPUT_DIR", out, "MODEL.FREEZE_BN", "False", "resume", os.path.join(out, "Aspp-1.pth"),
             "INPUT.INPUT_SIZE_TEST", "(193, 97)"], {"MI_SYNTH_LEN": "2"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Micro metric, val result: mIoU/mF1" in r.stderr + r.stdout


def test_bench_under_torchrun_nccl_single_rank_exercises_the_reducer():
    """The data-parallel code path (RCCL process group, bucketed all-reduce on a side HIP stream behind events, barrier,
    max-over-ranks timing) on the one GPU available: a single-rank `nccl` job with MI_DDP_FORCE=1 issues every collective."""
    import math
    r = run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29533",
             "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "161", "--batch", "2", "--no-cpu-baseline"],
            {"MI_DDP_FORCE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 1 and out["value"] > 0 and math.isfinite(out["config"]["final_loss"])
    # same run without the process group gives the same loss (the reducer averaged over one rank)
    r2 = run(["bench.py", "--steps", "3", "--warmup", "1", "--size", "161", "--batch", "2", "--no-cpu-baseline"], {})
    out2 = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][-1])
    assert abs(out2["config"]["final_loss"] - out["config"]["final_loss"]) < 1e-4


@pytest.mark.parametrize("workload,extra", [("pranet", ["--batch", "2", "--size", "96"]), ("gald", ["--batch", "1"]), ("deeplab_bn", ["--batch", "2", "--size", "161"]),
                                            ("fada", ["--batch", "2", "--size", "129"])])
def test_bench_other_workloads_print_the_contract_line(workload, extra):
    """bench.py --full --workload pranet | gald | deeplab_bn | fada (BASELINE config[3], the GALD step, the trainable-BatchNorm DeepLab step, config[4] on one GPU): one JSON
    line with the contract's keys, a roofline object for the dominant kernel of the instrumented steps, finite loss."""
    import math
    r = run(["bench.py", "--full", "--workload", workload, "--steps", "2", "--warmup", "1", "--no-cpu-baseline"] + extra, {})
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out, k
    assert out["value"] > 0 and out["steps"] == 2 and out["unit"] == "images/s" and "workload" in out["config"]
    assert out["roofline"]["bound"] in ("mfma", "hbm") and out["roofline"]["kernel"]
    loss = out.get("loss", out["config"].get("final_loss"))
    assert loss is not None and math.isfinite(loss)


def test_bench_plain_run_reports_the_timed_steps_and_dumps_the_last_one(tmp_path):
    """A plain bench.py run measures the timed steps only (no instrumented steps, no CPU baseline: those are --full), and `--dump-outputs DIR`
    writes what the last timed step computed - its loss, a seeded sample of the parameters and gradients it left - as float32 / float64 .npy
    files of 64 MB at most, the same in two runs (seeded inputs, formula weights)."""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / ("dump%d" % i)
        r = run(["bench.py", "--steps", "3", "--warmup", "1", "--size", "161", "--batch", "2", "--dump-outputs", str(d)], {})
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert out["steps"] == 3 and out["value"] > 0 and abs(out["ms_per_step"] * out["value"] - 2000) < 1
        assert not {"roofline", "kernels", "kernel_families", "cpu_baseline"} & set(out), sorted(out)
        arrs = {f: np.load(d / f) for f in os.listdir(d)}
        assert {"loss.npy", "feature_extractor_params.npy", "feature_extractor_grads.npy", "classifier_params.npy", "classifier_grads.npy"} <= set(arrs)
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
        assert sum(os.path.getsize(d / f) for f in arrs) <= 64 << 20
        assert abs(float(arrs["loss.npy"][0]) - out["config"]["final_loss"]) < 1e-4
        assert np.abs(arrs["feature_extractor_grads.npy"]).max() > 0 and np.abs(arrs["classifier_grads.npy"]).max() > 0
        dumps.append(arrs)
    for f, a in dumps[0].items():
        assert np.abs(a - dumps[1][f]).max() <= 1e-4 * np.abs(a).max(), f


def test_opt_in_kernel_variants_and_single_stream_schedule_stay_correct():
    """Selections of the product library that are not the default still have to be right: the 128-wide kernel on the shapes the ping-pong
    main loop normally takes (MI_IGEMM_PP=0), the tap-major contraction order, the 4-wave fused-row 3x3 weight gradient forced onto tiny
    shapes (MI_WGRAD_Q3=2; MI_WGRAD_Q3=0 = the per-tap kernel on the shapes the fused one normally takes), the 128 x 256 weight-gradient
    tile (MI_WGRAD_TI256=1), and the single-stream schedule (no forward lanes, weight gradients on the main stream) that bench.py's
    instrumented steps use.  (The kernels that did not win - the 256-wide tile of the 128-wide kernel, the shared-window 3x3 main loop, the
    8-wave fused-row weight gradient - are compiled only into experiment builds, tools/experiments/build.sh, since round 3.)
    Environment switches are read once per process, so each runs the relevant parity tests in a child pytest."""
    for env, sel, *reached in (({"MI_IGEMM_PP": "0"}, ["tests/test_gpu_ops.py", "-k", "full_size or identity"]),
                     ({"MI_IGEMM_PP_KORDER": "0"}, ["tests/test_gpu_ops.py", "-k", "identity or wide_tile"]),     # tap-major: bit-equal to the 128-wide kernel
                     ({"MI_WGRAD_Q3": "2"}, ["tests/test_gpu_ops.py", "-k", "conv_fwd_dgrad or fused_epilogue or tiny_and_ragged or wgrad_full or full_size_vs"]),
                     ({"MI_WGRAD_Q3": "0"}, ["tests/test_gpu_ops.py", "-k", "wgrad_full or full_size_vs"]),
                     ({"MI_WGRAD_S4": "0"}, ["tests/test_gpu_ops.py", "-k", "tiny_and_ragged or wgrad_full or pointwise or aspp_head_2048"]),   # 1x1 weight gradients on the double-buffer kernel
                     ({"MI_WGRAD_TI256": "0"}, ["tests/test_gpu_ops.py", "-k", "wgrad_full or aspp_head_2048 or aspp_head_upsample"]),   # the big 1x1 shapes on the 128 x 128 kernels
                     ({"MI_WGRAD_TI256": "1"}, ["tests/test_gpu_ops.py", "-k", "tiny_and_ragged or wgrad_full or full_size_vs or aspp_head_2048"]),
                     ({"MI_CHAIN": "all"}, ["tests/test_gpu_model.py", "-k", "r101_769 or hip_graph_replay"]),   # the 22 conv3 -> conv1 pairs of layer3 and their data gradients as one chained launch each
                     # measurement switches of experiment builds: the PRODUCT library must ignore them (they would skip main loops / stores)
                     ({"MI_GC_DBG": "7", "MI_GW_DBG": "1", "MI_P3_DBG": "31"}, ["tests/test_gpu_gops.py", "-k", "forward_and_batch_statistics or data_and_weight_gradient"]),
                     ({"MI_BN_TWO_PASS": "1"}, ["tests/test_gpu_bn.py", "-k", "tinynet_trainable"]),             # BatchNorm statistics as two passes
                     ({"MI_GWGRAD3": "2"}, ["tests/test_gpu_gops.py", "-k", "weight_gradient"]),                  # general family: fused-row weight gradient forced onto the small shapes
                     ({"MI_GWGRAD3": "0", "MI_INLAUNCH": "1", "MI_BN_INLAUNCH": "1"}, ["tests/test_gpu_gops.py", "tests/test_gpu_pranet.py", "-k", "weight_gradient or batch_statistics or graph_replay or running_statistics"]),   # per-tap kernel, in-launch reductions (opt-in since round 5)
                     ({"MI_GCONV_REMAP": "0"}, ["tests/test_gpu_pranet.py", "-k", "building_blocks or graph_replay or stale"]),     # tape: plain tile order
                     ({"MI_GCONV3_WGS": "1"}, ["tests/test_gpu_gops.py", "-k", "gconv"]),                                          # kernel-row window conv on every eligible (tiny) shape
                     ({"MI_GCONV_BN_ANY": "0", "MI_GCONV_KS2_WGS": "0", "MI_GCONV3_WGS": "0"}, ["tests/test_gpu_gops.py", "-k", "gconv"]),   # 32 / 64-wide tiles, one wave group, no window kernel
                     ({"MI_GCONV_BN_ANY": "0", "MI_GCONV_BN128": "1"}, ["tests/test_gpu_gconv_routes.py", "-s", "-k", "KC32_WGS or 1x7"],   # 128-wide tiles (>= 512 of them),
                      "gconv_kernel<128, 32, 8, 8, false, false, 1>", "gconv_kernel<128, 32, 8, 4, false, false, 1>"),                   # N = 256 and 334: they must be reached
                     ({"MI_BN_INLAUNCH": "1"}, ["tests/test_gpu_pranet.py", "-k", "building_blocks"]),     # the tape's in-launch finalize (only host/pranet.py reads the switch;
                                                                                                              # test_gpu_gops.py runs mi_gconv_bn itself, a 64-wide launch included)
                     ({"MI_GCONV_BN32_WGS": "0", "MI_GCONV_BN_FORCE": "16"}, ["tests/test_gpu_gops.py", "-k", "forward_and_batch_statistics or data_and_weight_gradient"]),   # every width forced onto the small ragged shapes
                     ({"MI_GCONV_BN32_WGS": "0", "MI_GCONV_BN_FORCE": "64"}, ["tests/test_gpu_gops.py", "-k", "forward_and_batch_statistics or data_and_weight_gradient"]),
                     ({"MI_GCONV_BN32_WGS": "0", "MI_GCONV_BN_FORCE": "80"}, ["tests/test_gpu_gops.py", "-k", "forward_and_batch_statistics or data_and_weight_gradient"]),
                     ({"MI_GCONV_BN32_WGS": "0", "MI_GCONV_BN_FORCE": "112"}, ["tests/test_gpu_gops.py", "-k", "forward_and_batch_statistics or data_and_weight_gradient"]),
                     ({"MI_GWM_STEPS": "4", "MI_GWM_FUSED3": "0"}, ["tests/test_gpu_gops.py", "-k", "many_convs"]),                # batched weight gradients: many K splits, the one-conv fusing rule
                     ({"MI_WGRAD_STREAM": "0", "MI_BATCH_LANES": "1"}, ["tests/test_gpu_model.py", "-k", "tinynet"])):
        r = run(["-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider"] + sel, env)
        assert r.returncode == 0, (env, r.stdout[-3000:])
        assert " passed" in r.stdout and " failed" not in r.stdout
        for route in reached:                                # (routes the child run must have launched, as tests/test_gpu_gconv_routes.py prints them)
            assert route in r.stdout, (env, route)


def test_rccl_entry_points_of_the_cabi_single_rank_communicator():
    """mi_comm_unique_id / mi_comm_init_rank / mi_allreduce_bucket / mi_comm_destroy (include/mi355seg.h): the
    exchange a non-Python host drives itself.  One rank is all this box has: a 1-rank communicator must return the bucket
    unchanged for sum and for average, fp32 and bf16, on a side stream, and report errors as codes."""
    code = r'''
import ctypes, torch
from rnd_semantic_segmentation_amd import _lib
L = _lib.lib()
uid = ctypes.create_string_buffer(128)
assert L.mi_comm_unique_id(uid) == 0, L.mi_last_error()
comm = ctypes.c_void_p()
assert L.mi_comm_init_rank(ctypes.byref(comm), 1, uid, 0) == 0, L.mi_last_error()
side = torch.cuda.Stream()
for dtype, code_ in ((torch.float32, 0), (torch.bfloat16, 1)):
    x = (torch.arange(100003, device="cuda") % 251).to(dtype)
    want = x.clone()
    ev = torch.cuda.Event(); ev.record(); side.wait_event(ev)
    for avg in (0, 1):
        assert L.mi_allreduce_bucket(ctypes.c_void_p(x.data_ptr()), x.numel(), code_, avg, comm, ctypes.c_void_p(side.cuda_stream)) == 0, L.mi_last_error()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x, want), dtype
assert L.mi_allreduce_bucket(None, 4, 0, 0, comm, None) == -22
assert L.mi_allreduce_bucket(ctypes.c_void_p(16), 4, 7, 0, comm, None) == -22 and b"dtype" in L.mi_last_error()
assert L.mi_comm_destroy(comm) == 0
print("rccl c-abi ok")
'''
    r = run(["-c", code], {})
    assert r.returncode == 0 and "rccl c-abi ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_pranet_train_src_then_test_py_roundtrip(tmp_path):
    """BASELINE config[3] through the unchanged scripts: `train_src.py --model pranet -cfg configs/pranet_src_polyp.yaml` (reference
    train_src.py:29-30) trains PraNet on synthetic polyp crops - three passes per batch, warm-up schedule, PraNet-<epoch>.pth with the
    reference's checkpoint keys - and `test.py -c renders/kvasir.json` (reference test.py:35-36) resumes from it and prints the meters."""
    out = str(tmp_path / "pranet") + "/"
    r = run(["train_src.py", "--model", "pranet", "-cfg", "configs/pranet_src_polyp.yaml", "OUTPUT_DIR", out, "SOLVER.EPOCHS", "2", "SOLVER.CHECKPOINT_PERIOD", "1",
             "SOLVER.BATCH_SIZE", "2", "INPUT.TRAINSIZE", "96"], {"MI_SYNTH_LEN": "4"})
    assert r.returncode == 0, r.stderr[-3000:]
    log = r.stderr + r.stdout
    assert "lateral-2:" in log and "learning_rate: 0.00001250" in log and "learning_rate: 0.00003000" in log       # BASE_LR / 8, then warm-up step 1
    ck = torch.load(os.path.join(out, "PraNet-2.pth"), map_location="cpu")
    assert set(ck) == {"epoch", "model", "optimizer"} and ck["epoch"] == 2 and len(ck["model"]) == 922
    assert int(ck["model"]["resnet.bn1.num_batches_tracked"]) == 12                                                 # 2 epochs x 2 batches x 3 passes
    assert set(ck["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(ck["optimizer"]["state"][0]["step"]) == 12
    r = run(["test.py", "-cfg", "configs/pranet_src_polyp.yaml", "-c", "renders/kvasir.json", "OUTPUT_DIR", out, "resume", os.path.join(out, "PraNet-2.pth"),
             "INPUT.INPUT_SIZE_TEST", "(96, 96)"], {"MI_SYNTH_LEN": "3"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Micro metric, val result: mIoU/mF1" in r.stderr + r.stdout


def test_gald_train_src_roundtrip(tmp_path):
    """`train_src.py --model gald -cfg configs/gald_src.yaml` (reference train_src.py:33-34, the model run.sh launches): HarDNet-68 + GCPA decoder
    trained on synthetic crops, poly learning rate, Gald-<epoch>.pth with the reference's checkpoint keys, gald_chart_params.json."""
    out = str(tmp_path / "gald")
    r = run(["train_src.py", "--model", "gald", "-cfg", "configs/gald_src.yaml", "OUTPUT_DIR", out, "SOLVER.EPOCHS", "1", "SOLVER.CHECKPOINT_PERIOD", "1",
             "SOLVER.BATCH_SIZE", "2", "INPUT.SOURCE_INPUT_SIZE_TRAIN", "(256, 224)"], {"MI_SYNTH_LEN": "6"})
    assert r.returncode == 0, r.stderr[-3000:]
    chart = json.load(open(os.path.join(out, "gald_chart_params.json")))
    assert len(chart["loss"]) == 3 and all(0 < v < 20 for v in chart["loss"]) and chart["learning rate"][0] == 1e-4
    ck = torch.load(os.path.join(out, "Gald-1.pth"), map_location="cpu")
    assert set(ck) == {"epoch", "iteration", "encoder", "decoder", "optimizer_enc", "optimizer_dec"} and ck["iteration"] == 3
    assert len(ck["encoder"]) == 404 and len(ck["decoder"]) == 186
    assert int(ck["encoder"]["hardnet.base.0.norm.num_batches_tracked"]) == 3
    # evaluation through the unchanged script (reference test.py:39-40: a render json whose name starts with "gald" picks GALDTester): fp32 by default
    r = run(["test.py", "-cfg", "configs/gald_src.yaml", "-c", "renders/cityscapes_gald.json", "OUTPUT_DIR", out, "resume", os.path.join(out, "Gald-1.pth"),
             "INPUT.INPUT_SIZE_TEST", "(256, 224)"], {"MI_SYNTH_LEN": "2"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Micro metric, val result: mIoU/mF1" in r.stderr + r.stdout
    cm = json.load(open(os.path.join(out, "gald_confusion_matrix.json")))
    assert len(cm["cmt"]) == 19 and len(cm["classes"]) == 19 and sum(map(sum, cm["cmt"])) > 0
