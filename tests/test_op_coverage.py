"""Every symbol include/vqa_hot.h declares is named in some GPU test (tests/test_gpu_*.py, as vqa_x or as the word x),
or is listed below with the reason it needs no op-level test of its own.  A kernel whose op test is deleted, or a new
entry point added without one, fails here."""
import glob
import os
import re

# symbol -> why no tests/test_gpu_*.py names it.  Kernels pinned under another name point at the test that runs them.
ALLOWED = {
    # version, errors, report keys and workspace / layout queries: host-only (tests/test_abi.py, tests/test_sanitizers.py)
    "vqa_hot_version": "host-only query, tests/test_abi.py",
    "vqa_hot_error_string": "host-only query, tests/test_abi.py",
    "vqa_report_key": "host-only table, tests/test_abi.py",
    "vqa_pretrain_report_key": "host-only table, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_fusion_workspace_bytes": "host-only layout query, tests/test_abi.py",
    "vqa_fusion_tensor": "host-only layout query, tests/test_abi.py",
    "vqa_fusion_gru_form": "host-only query of the step's recurrence form, tests/test_encoder_routes_host.py",
    "vqa_pretrain_workspace_bytes": "host-only layout query, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_pretrain_tensor": "host-only layout query, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_gemm_bf16x3_workspace_floats": "host-only size query behind ops.gemm_bf16x3_ex (test_gpu_ops.py)",
    # knobs, debug and profiling hooks
    "vqa_gemm_bf16x3_set_mode": "tuning knob of the experimental bf16x3 GEMM",
    "vqa_gemm_shortk_set_mode": "tuning knob of the short-K GEMM",
    "vqa_gru_set_persistent": "A/B switch of the recurrence forms",
    "vqa_gru_persistent_set_census": "debug stamp of the persistent recurrence",
    "vqa_gru_ws_set_form": "A/B switch of the weight-stationary recurrence",
    "vqa_gru_ws_set_stamps": "debug stamp of the weight-stationary recurrence",
    "vqa_probe_enable": "profiling probe, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_probe_disable": "profiling probe, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_probe_labels": "profiling probe, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_probe_read": "profiling probe, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_probe_read_label": "profiling probe, tests/host_abi_exercise.py (run by tests/test_sanitizers.py)",
    "vqa_roctx_enable": "profiler markers",
    "vqa_clock_sample": "clock measurement of the benchmark",
    "vqa_stream_delay_us": "timing aid: a wave polls the real-time counter",
    "vqa_graph_capture_abort": "graph-capture error path (test_gpu_graph.py covers capture and replay)",
    # whole-model entry points (test_gpu_pretrain.py / test_gpu_fusion.py call them through the model classes)
    "vqa_pretrain_forward": "whole-model entry point, test_gpu_pretrain.py",
    # kernels pinned under another name
    "vqa_gemm_bf16x3_nn": "ops.gemm_bf16x3, test_gpu_ops.py::test_experimental_bf16x3_gemm_is_f32_equivalent",
    "vqa_gemm_shortk_nn": "ops.gemm_shortk, test_gpu_ops.py::test_shortk_gemm_matches_float64",
    "vqa_gru_fill_finished": "vqa_gru_seq_fwd_live's finished rows, test_gpu_gru_f64.py (form live)",
    "vqa_gru_zero_finished": "vqa_gru_seq_bwd_live's finished rows, test_gpu_gru_f64.py (form live: dxp exactly 0)",
}

# the kernels tests/test_gpu_rowops_f64.py pins to a float64 reference: they must stay named THERE
ROWOPS = [
    "reverse_tokens", "bi_outputs_fwd", "bi_outputs_bwd", "bi_dx_combine",
    "reparam_fwd", "reparam_bwd", "outer_rows", "tile_mul_fwd", "tile_mul_bwd", "marginal_entropy", "extra_report",
    "embed2_fwd", "embed2_bwd", "lstm_step_fwd", "lstm_step_bwd", "relu_fwd", "relu_bwd", "score_fwd", "score_bwd",
    "ln_act_fwd", "ln_act_bwd", "mul", "mul_bwd", "tanh_bwd", "add_inplace", "embed_bwd_len_det",
    "report_reduce", "sumsq", "clip_adam", "clip_adam_dev", "adam_lr_step",
    "gru_gates_fwd", "gru_cand_fwd", "gru_bwd_a", "gru_bwd_b", "im2col_nhwc",
]

# the attention entry points tests/test_gpu_attn_f64.py pins to the float64 reference of tests/attn_ref.py, form by form
ATTN = ["attn_pool_fwd", "attn_pool_bwd", "attn_pool_fwd_rep", "attn_pool_bwd_rep"]

# the f32 GEMM entry points and knobs tests/test_gpu_gemm_f64.py pins to the float64 reference of tests/gemm_ref.py, route by route
GEMM = ["gemm_f32", "gemm_f32_ex", "gemm_f32_gather", "gemm_set_config", "gemm_set_order", "gemm_set_max_blocks",
        "gemm_set_tall_config", "gemm_workspace_floats"]

# the mixed-precision GEMM entry points tests/test_gpu_gemm_bf16_f64.py pins to the float64 reference of tests/gemm_bf16_ref.py, route by route
GEMM_BF16 = ["gemm_bf16", "gemm_bf16_a16", "gemm_bf16_workspace_floats"]

# the f32 extractor entry points and knobs tests/test_gpu_conv_f64.py pins to the float64 reference of tests/conv_ref.py, route by route
CONV = ["conv2d_nhwc", "conv2d_nhwc_bwd", "conv2d_bwd_workspace_floats", "conv_set_config", "pad_c3c4_nhwc",
        "maxpool3x3s2_same_nhwc", "subsample_nhwc", "crop_and_resize_nhwc"]

# the loss heads and the paired LayerNorm tests/test_gpu_loss_f64.py pins to the float64 references of tests/loss_ref.py, route by route
LOSS = ["loss_fwd", "loss2_fwd", "rowmin_mask_fwd", "rowmin_mask_bwd", "softmax_ce_fwd", "softmax_ce_pair_fwd",
        "softmax_set_fast", "ln_pair_mul_fwd", "ln_pair_mul_bwd", "ln_pair_mul_supported"]


def _declared(repo_root):
    src = open(os.path.join(repo_root, "include", "vqa_hot.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vqa_[a-z0-9_]+)\s*\(", src)))


def _named(name, text):
    return re.search(r"\b%s\b" % name, text) is not None or re.search(r"\b%s\b" % name[len("vqa_"):], text) is not None


def test_every_declared_symbol_has_a_gpu_test_or_a_reason(repo_root):
    names = _declared(repo_root)
    texts = [open(f).read() for f in sorted(glob.glob(os.path.join(repo_root, "tests", "test_gpu_*.py")))]
    untested = [n for n in names if n not in ALLOWED and not any(_named(n, t) for t in texts)]
    assert not untested, "named in no tests/test_gpu_*.py and not in ALLOWED: %s" % untested
    stale = sorted(set(ALLOWED) - set(names))
    assert not stale, "ALLOWED lists symbols the header no longer declares: %s" % stale


def test_the_row_kernels_stay_pinned_by_their_float64_test(repo_root):
    text = open(os.path.join(repo_root, "tests", "test_gpu_rowops_f64.py")).read()
    calls = set(re.findall(r"\"(vqa_[a-z0-9_]+)\"", text))
    missing = ["vqa_" + k for k in ROWOPS if "vqa_" + k not in calls]
    assert not missing, "tests/test_gpu_rowops_f64.py no longer calls %s" % missing
    assert not set("vqa_" + k for k in ROWOPS) & set(ALLOWED)
    declared = set(_declared(repo_root))
    assert all("vqa_" + k in declared for k in ROWOPS)


def test_the_attention_kernels_stay_pinned_by_their_float64_test(repo_root):
    text = open(os.path.join(repo_root, "tests", "test_gpu_attn_f64.py")).read()
    calls = set(re.findall(r"\bvqa_[a-z0-9_]+\b", text))
    missing = ["vqa_" + k for k in ATTN if "vqa_" + k not in calls]
    assert not missing, "tests/test_gpu_attn_f64.py no longer calls %s" % missing
    assert "vqa_attn_set_fast" in calls and "attn_ref" in text
    assert not set("vqa_" + k for k in ATTN) & set(ALLOWED)
    declared = set(_declared(repo_root))
    assert all("vqa_" + k in declared for k in ATTN)


def test_the_f32_gemm_stays_pinned_by_its_float64_test(repo_root):
    text = open(os.path.join(repo_root, "tests", "test_gpu_gemm_f64.py")).read()
    calls = set(re.findall(r"\blib\.(vqa_[a-z0-9_]+)\(", text))
    missing = ["vqa_" + k for k in GEMM if "vqa_" + k not in calls]
    assert not missing, "tests/test_gpu_gemm_f64.py no longer calls %s" % missing
    assert "vqa_gemm_shortk_set_mode" in calls and "gemm_ref" in text
    assert not set("vqa_" + k for k in GEMM) & set(ALLOWED)
    declared = set(_declared(repo_root))
    assert all("vqa_" + k in declared for k in GEMM)


def test_the_bf16_gemm_stays_pinned_by_its_float64_test(repo_root):
    text = open(os.path.join(repo_root, "tests", "test_gpu_gemm_bf16_f64.py")).read()
    calls = set(re.findall(r"\blib\.(vqa_[a-z0-9_]+)\(", text))
    missing = ["vqa_" + k for k in GEMM_BF16 if "vqa_" + k not in calls]
    assert not missing, "tests/test_gpu_gemm_bf16_f64.py no longer calls %s" % missing
    assert "gemm_bf16_ref" in text
    assert not set("vqa_" + k for k in GEMM_BF16) & set(ALLOWED)
    declared = set(_declared(repo_root))
    assert all("vqa_" + k in declared for k in GEMM_BF16)


def test_the_f32_extractor_kernels_stay_pinned_by_their_float64_test(repo_root):
    text = open(os.path.join(repo_root, "tests", "test_gpu_conv_f64.py")).read()
    calls = set(re.findall(r"\blib\.(vqa_[a-z0-9_]+)\(", text))
    missing = ["vqa_" + k for k in CONV if "vqa_" + k not in calls]
    assert not missing, "tests/test_gpu_conv_f64.py no longer calls %s" % missing
    assert {"vqa_gemm_set_config", "vqa_gemm_shortk_set_mode", "vqa_gemm_shortk_supported"} <= calls and "conv_ref" in text
    assert not set("vqa_" + k for k in CONV) & set(ALLOWED)
    declared = set(_declared(repo_root))
    assert all("vqa_" + k in declared for k in CONV)


def test_the_loss_heads_and_the_paired_layernorm_stay_pinned_by_their_float64_test(repo_root):
    text = open(os.path.join(repo_root, "tests", "test_gpu_loss_f64.py")).read()
    calls = set(re.findall(r"\"(vqa_[a-z0-9_]+)\"", text)) | set(re.findall(r"\blib\.(vqa_[a-z0-9_]+)\(", text))
    missing = ["vqa_" + k for k in LOSS if "vqa_" + k not in calls]
    assert not missing, "tests/test_gpu_loss_f64.py no longer calls %s" % missing
    assert "vqa_report_reduce" in calls and "loss_ref" in text
    assert not set("vqa_" + k for k in LOSS) & set(ALLOWED)
    declared = set(_declared(repo_root))
    assert all("vqa_" + k in declared for k in LOSS)
