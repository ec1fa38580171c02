"""Host-only exercise of libvqahot's dispatch layer: every path that runs BEFORE a kernel launch -- argument validation,
workspace layouts, named-tensor lookups, report keys, probe bookkeeping.  No GPU is touched.  Run directly, or by
tests/test_sanitizers.py against the ASan + UBSan build (csrc/build.py --sanitize) with the ASan runtime preloaded:

    python tests/host_abi_exercise.py [path/to/libvqahot(.so | _asan.so)]
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vqa_transfer_externaldata_amd import _lib  # noqa: E402

if len(sys.argv) > 1:
    _lib._LIB_PATH = os.path.abspath(sys.argv[1])
lib = _lib.load()
checks = 0


def ok(cond, what):
    global checks
    checks += 1
    if not cond:
        raise SystemExit("host ABI exercise failed: " + what)


ok(lib.vqa_hot_version() == _lib.ABI_VERSION, "version")
ok(lib.vqa_hot_error_string(0) == b"ok" and lib.vqa_hot_error_string(-99) is not None, "error strings")
ok([lib.vqa_report_key(i) is not None for i in range(-2, 16)] == [False] * 2 + [True] * 13 + [False] * 3, "report keys")
ok([lib.vqa_pretrain_report_key(i) is not None for i in range(-1, 15)] == [False] + [True] * 13 + [False] * 2, "pretrain keys")
PRETRAIN_KEYS = [b"obj_blank_fill_loss", b"obj_blank_fill_acc", b"obj_blank_fill_top_5_acc", b"obj_wordset_loss", b"obj_wordset_acc",
                 b"obj_wordset_top_5_acc", b"attr_blank_fill_loss", b"attr_blank_fill_acc", b"attr_blank_fill_top_5_acc",
                 b"attr_wordset_loss", b"attr_wordset_acc", b"attr_wordset_top_5_acc", b"total_loss"]
ok([lib.vqa_pretrain_report_key(i) for i in range(14)] == PRETRAIN_KEYS + [None], "pretrain key names")

# fusion model: workspace + every named tensor, for all five model types and a sweep of sizes (ragged, tiny, full)
off, n = C.c_int64(), C.c_int64()
names = [b"V_ft", b"num_V_ft", b"v_linear_v", b"condition", b"q_linear_v", b"att_score", b"pooled_V_ft", b"pooled_linear_l",
         b"l_linear_l", b"joint", b"logit", b"pred", b"stats", b"report", b"dlogit", b"dx_embed", b"hs", b"xp", b"x_tm"]
VARIANT_TENSORS = {4: [b"logit_fixed", b"logit_tuned", b"dlogit_tuned"], 6: [b"logit_fixed", b"logit_tuned", b"dlogit_tuned", b"logit_raw", b"rowmin"],
                   5: [b"l_joint", b"pre_jl"], 7: [b"q_L_ft2", b"pre_ft2", b"d_ft2"], 8: [b"q_L_mean", b"d_qm"], 9: [b"v_adapt", b"pre_va", b"d_va"],
                   10: [b"q_L_mean", b"q_L_log_sigma_sq", b"q_L_mean_noise", b"extra_row"],
                   11: [b"tile_in", b"pre_tj", b"tile_joint", b"tile_z", b"marginal_prob", b"extra_row", b"d_tile_in"],
                   12: [b"q_rev", b"hs_bw", b"q_L_map", b"q_L_ft", b"q_att_key", b"w_att_score", b"q_v_ft", b"pooled_q_v", b"d_e2", b"dxp_bw"],
                   13: [b"lv_gq", b"lv_hsa", b"q_map_V", b"pooled_map_L", b"lv_al", b"lv_dga", b"q_L_ft", b"answer_ft"]}
for mt in range(14):
    for (B, R, D, H, T, W, A, Vq, N) in ((1, 1, 4, 4, 1, 1, 1, 1, 1), (5, 6, 24, 16, 7, 12, 21, 30, 9),
                                         (7, 36, 64, 32, 3, 300, 50, 60, 16), (512, 36, 2048, 1024, 14, 300, 3000, 16384, 8192)):
        if mt == 12 and H % 8:
            continue                      # the bi-directional encoder needs two 16-byte-row halves
        if mt == 13 and (W % 4 or Vq <= 3):
            continue
        d = _lib.Dims(B=B, R=R, D=D, H=H, T=T, W=W, A=A, Vq=Vq, N_img=N, model_type=mt, keep_att=0.8, keep_joint=0.5,
                      inv_global_batch=1.0 / B, num_marginal=200 if mt == 11 else 0, ent_cols=min(A, 2272) if mt == 11 else 0,
                      extra_weight=0.1, map_dim=H if mt == 13 else 0, La=4 if mt == 13 else 0)
        total = lib.vqa_fusion_workspace_bytes(C.byref(d))
        ok(total > 0, "workspace bytes %r" % ((mt, B),))
        for nm in names + VARIANT_TENSORS.get(mt, []):
            ok(lib.vqa_fusion_tensor(C.byref(d), nm, C.byref(off), C.byref(n)) == 0, "tensor %s" % nm)
            ok(off.value % 16 == 0 and 0 <= off.value and off.value + 4 * n.value <= total, "tensor %s inside the workspace" % nm)
        ok(lib.vqa_fusion_tensor(C.byref(d), b"logit_tuned", C.byref(off), C.byref(n)) == (0 if mt in (4, 6) else -1), "variant tensor")
        ok(lib.vqa_fusion_tensor(C.byref(d), b"", C.byref(off), C.byref(n)) == -1, "empty name")
        ok(lib.vqa_fusion_tensor(C.byref(d), b"x" * 300, None, None) == -1, "long unknown name")
for bad in (dict(B=0), dict(R=0), dict(model_type=14), dict(model_type=-1), dict(H=-4), dict(N_img=0), dict(model_type=12, H=12),
            dict(model_type=13), dict(model_type=13, map_dim=8), dict(model_type=13, map_dim=8, La=2, Vq=3),
            dict(model_type=11), dict(model_type=11, num_marginal=3), dict(model_type=11, num_marginal=3, ent_cols=5),
            dict(model_type=11, num_marginal=1 << 28, ent_cols=4), dict(model_type=11, num_marginal=2, ent_cols=4097, A=5000)):
    kw = dict(B=4, R=4, D=8, H=8, T=2, W=4, A=4, Vq=4, N_img=4, model_type=0)
    kw.update(bad)
    ok(lib.vqa_fusion_workspace_bytes(C.byref(_lib.Dims(**kw))) < 0, "bad dims %r" % (bad,))
ok(lib.vqa_fusion_workspace_bytes(None) < 0 and lib.vqa_fusion_tensor(None, b"logit", None, None) < 0, "null dims")

# entry points with null / undersized arguments: rejected before any launch
d = _lib.Dims(B=4, R=4, D=8, H=8, T=2, W=4, A=4, Vq=4, N_img=4, model_type=0, keep_att=0.8, keep_joint=0.5, inv_global_batch=0.25)
ok(lib.vqa_fusion_forward(C.byref(d), None, None, None, 0, 1, None) == -1, "forward null")
p, b = _lib.Params(), _lib.Batch()
ok(lib.vqa_fusion_forward(C.byref(d), C.byref(p), C.byref(b), C.c_void_p(4096), 16, 1, None) == -5, "forward small workspace")
ok(lib.vqa_fusion_backward_phases(C.byref(d), C.byref(p), C.byref(p), C.byref(b), None, 0, None, 15, None) == -1, "backward null")
ok(lib.vqa_gemm_f32(1, 1, 4, 4, 4, 16, 4, 16, 4, 16, 4, None, None, 0, 0, None, 0, None) == -4, "gemm TT")
ok(lib.vqa_gemm_f32(0, 0, 4, 4, 4, None, 4, None, 4, None, 4, None, None, 0, 0, None, 0, None) == -1, "gemm null")
ok(lib.vqa_ln_relu_fwd(None, None, None, None, 1.0, None, None, None, 1, 1, 4, None) == -1, "ln null")
ok(lib.vqa_loss2_fwd(None, None, None, None, None, None, None, 1.0, None, None, None, None, None, 0, 1, 4, None) == -1, "loss2 null")
ok(lib.vqa_rowmin_mask_fwd(None, None, None, None, 1, 4, None) == -1 and lib.vqa_rowmin_mask_bwd(None, None, None, None, 1, 4, None) == -1, "rowmin null")
for M, N, K in ((1, 1, 1), (512, 3000, 2048), (18432, 1024, 2048), (7168, 300, 3072), (10240, 4000, 2048)):
    for tA, tB in ((0, 0), (0, 1), (1, 0)):
        for sk in (0, 1, 3, 8):
            ok(lib.vqa_gemm_workspace_floats(tA, tB, M, N, K, sk) >= 0, "gemm workspace")
ok(lib.vqa_conv2d_bwd_workspace_floats(128, 28, 28, 128, 3, 3, 128, 8) > lib.vqa_conv2d_bwd_workspace_floats(128, 28, 28, 128, 3, 3, 128, 1) > 0,
   "conv bwd workspace grows with the chunk")
ok(lib.vqa_conv2d_bwd_workspace_floats(0, 1, 1, 4, 1, 1, 4, 1) < 0, "conv bwd workspace bad dims")
ok(lib.vqa_conv2d_nhwc_bwd(None, 1, 4, 4, 4, None, 1, 1, 4, 1, 0, 0, 4, 4, None, None, 0, None, None, None, None, None, None, 0, None) == -1,
   "conv bwd null")
ok(lib.vqa_conv2d_nhwc_bwd(C.c_void_p(4096), 1, 4, 4, 4, C.c_void_p(4096), 1, 1, 4, 1, 0, 0, 4, 4, None, None, 1, C.c_void_p(4096), None, None,
                           None, None, C.c_void_p(4096), 1 << 20, None) == -1, "conv bwd relu without y")
ok(lib.vqa_conv2d_nhwc_bwd(C.c_void_p(4096), 1, 4, 4, 3, C.c_void_p(4096), 1, 1, 4, 1, 0, 0, 4, 4, None, None, 0, C.c_void_p(4096), None, None,
                           None, None, C.c_void_p(4096), 1 << 20, None) == -2, "conv bwd Ci % 4")
ok(lib.vqa_conv2d_nhwc_bwd(C.c_void_p(4096), 4, 8, 8, 8, C.c_void_p(4096), 3, 3, 8, 1, 1, 1, 8, 8, None, None, 0, C.c_void_p(4096), None, None,
                           None, None, C.c_void_p(4096), 16, None) == -5, "conv bwd workspace too small")
ok(lib.vqa_colsum_workspace_floats(1, 1) >= 0 and lib.vqa_colsum_workspace_floats(25600, 2048) > 0, "colsum workspace")
ok(lib.vqa_sumsq_workspace_floats(0) >= 0 and lib.vqa_sumsq_workspace_floats(1 << 30) > 0, "sumsq workspace")

# cfg-5 model: layouts for both LayerNorm modes, ragged sizes
pnames = [b"report", b"S/z", b"S/dz", b"S/pooled", b"J/hs", b"J/xp", b"dxp", b"wx_cat"] + \
    [("%s/%s" % (k, t)).encode() for k in ("obj", "attr") for t in ("att", "pooled", "v", "qv", "valid", "bf/z", "ws/z", "bf/j", "ws/ll", "bf/vl")]
for flags in (0, 4, 5):
    for (B, n_, R, D, H, W, A, Vq, nws, L) in ((1, 1, 1, 4, 4, 1, 1, 1, 1, 1), (3, 5, 6, 16, 8, 12, 12, 20, 7, 4),
                                               (512, 5, 36, 2048, 1024, 300, 4000, 5000, 2000, 10)):
        pd = _lib.PtDims(B=B, n=n_, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=nws, L=L, flags=flags, keep_att=0.8, keep_joint=0.5)
        total = lib.vqa_pretrain_workspace_bytes(C.byref(pd))
        ok(total > 0, "pretrain workspace")
        for nm in pnames:
            ok(lib.vqa_pretrain_tensor(C.byref(pd), nm, C.byref(off), C.byref(n)) == 0, "pretrain tensor %s" % nm)
            ok(off.value + 4 * n.value <= total and off.value >= 0, "pretrain tensor %s inside" % nm)
        ok(lib.vqa_pretrain_tensor(C.byref(pd), b"nope", C.byref(off), C.byref(n)) == -1, "pretrain unknown")
        # the cfg-5 entry points are the bf | ws case of the variable-head-set path: same layout, name by name
        xd = _lib.PtExtDims(base=pd, heads=3, Lc=0, n_ctx=0)
        ok(total == lib.vqa_pretrain_ext_workspace_bytes(C.byref(xd)), "pretrain workspace == ext workspace, heads 3")
        xoff, xn = C.c_int64(), C.c_int64()
        for nm in pnames + [b"d_lft", b"d_pooled", b"obj/ws/stats", b"attr/bf/j_mean"]:
            ok(lib.vqa_pretrain_tensor(C.byref(pd), nm, C.byref(off), C.byref(n)) == 0 and
               lib.vqa_pretrain_ext_tensor(C.byref(xd), nm, C.byref(xoff), C.byref(xn)) == 0, "pretrain / ext tensor %s" % nm)
            ok((off.value, n.value) == (xoff.value, xn.value), "pretrain tensor %s == ext tensor" % nm)
ok(lib.vqa_pretrain_workspace_bytes(C.byref(_lib.PtDims(B=1, n=9, R=1, D=4, H=4, W=1, A=1, Vq=1, n_ws=1, L=1))) < 0, "n > 8")
ok(lib.vqa_pretrain_forward(None, None, None, None, 0, 1, None) == -1, "pretrain forward null")
pd = _lib.PtDims(B=2, n=5, R=6, D=16, H=8, W=12, A=12, Vq=20, n_ws=7, L=4, keep_att=0.8, keep_joint=0.5)
ok(lib.vqa_pretrain_backward_phases(C.byref(pd), C.byref(_lib.PtParams()), C.byref(_lib.PtParams()), C.byref(_lib.PtBatch()),
                                    C.c_void_p(4096), 1 << 40, None, 0, None) == -1, "phases = 0")
ok(lib.vqa_pretrain_backward_phases(C.byref(pd), C.byref(_lib.PtParams()), C.byref(_lib.PtParams()), C.byref(_lib.PtBatch()),
                                    C.c_void_p(4096), 1 << 40, None, 16, None) == -1, "phases = 16")

# probe bookkeeping (no scope runs without a launch: labels only)
ok(lib.vqa_probe_enable(None, 4) == -1 and lib.vqa_probe_enable(b"", 4) == -1 and lib.vqa_probe_enable(b"a", 0) == -1, "probe args")
ok(lib.vqa_probe_enable(b"gru.fwd,,gru.bwd,gru.fwd,*", 3) in (0, -3), "probe enable (events need a device: -3 without one)")
buf = C.create_string_buffer(8)
need = lib.vqa_probe_labels(buf, 8)
ok(need >= 1 and len(buf.value) <= 7, "probe labels truncated safely")
ms, cnt = (C.c_float * 4)(), C.c_int()
ok(lib.vqa_probe_read_label(b"not.there", ms, 4, C.byref(cnt)) == 0 and cnt.value == 0, "probe read unknown label")
ok(lib.vqa_probe_read(ms, 4, C.byref(cnt)) == 0 and cnt.value == 0, "probe read first label")
ok(lib.vqa_probe_read(None, 4, C.byref(cnt)) == -1, "probe read null")
ok(lib.vqa_probe_disable() == 0 and lib.vqa_probe_disable() == 0, "probe disable twice")
ok(lib.vqa_roctx_enable(0) == 0, "roctx off")

# round-3 entry points: shape predicates and argument validation (everything that returns before a launch)
for (M, N, K, lda, ldb, ldc, want) in ((7168, 3072, 300, 304, 3072, 3072, 1), (128, 64, 308, 308, 64, 64, 1), (128, 64, 516, 516, 64, 64, 0), (128, 48, 64, 64, 48, 48, 0),
                                       (128, 64, 62, 64, 64, 64, 0), (128, 64, 64, 66, 64, 64, 0), (0, 64, 64, 64, 64, 64, 0),
                                       (128, 64, 64, 60, 64, 64, 0), (128, 64, 64, 64, 32, 64, 0), (128, 64, 64, 64, 64, 32, 0),
                                       (1 << 30, 64, 64, 64, 64, 64, 0), (100, 32, 4, 4, 32, 32, 1)):
    ok(lib.vqa_gemm_shortk_supported(M, N, K, lda, ldb, ldc) == want, "shortk supported %r" % ((M, N, K, lda, ldb, ldc),))
ok(lib.vqa_gemm_shortk_nn(128, 64, 64, None, 64, None, 64, None, 64, None, None, None, 0, 0, None) == -1, "shortk null operands")
ok(lib.vqa_gemm_shortk_nn(128, 64, 516, C.c_void_p(4096), 516, C.c_void_p(4096), 64, C.c_void_p(4096), 64, None, None, None, 0, 0,
                          None) == -4, "shortk K too large")
ok(lib.vqa_gemm_shortk_nn(128, 64, 64, C.c_void_p(4100), 64, C.c_void_p(4096), 64, C.c_void_p(4096), 64, None, None, None, 0, 0,
                          None) == -2, "shortk misaligned A")
ok(lib.vqa_gemm_shortk_nn(128, 64, 64, C.c_void_p(4096), 64, C.c_void_p(4096), 64, C.c_void_p(4096), 64, None, None, C.c_void_p(4096),
                          32, 0, None) == -1, "shortk residual rows too short")
ok(lib.vqa_gemm_shortk_set_grid(-5) == 0 and lib.vqa_gemm_shortk_set_grid(0) == 0, "shortk grid override")
ok(lib.vqa_gemm_shortk_set_mode(7) == 0 and lib.vqa_gemm_shortk_set_mode(-1) == 0, "shortk mode")
for (M, N, K, want) in ((256, 256, 2048, 1), (250, 256, 2048, 0), (256, 200, 2048, 0), (256, 256, 2040, 0), (0, 128, 32, 0)):
    ok(lib.vqa_gemm_bf16x3_supported(M, N, K) == want, "bf16x3 supported %r" % ((M, N, K),))
ok(lib.vqa_gemm_bf16x3_workspace_floats(256, 128, 4096, 4) == 4 * 256 * 128 and lib.vqa_gemm_bf16x3_workspace_floats(256, 128, 4096, 1) == 0,
   "bf16x3 workspace")
ok(lib.vqa_gemm_bf16x3(0, 256, 256, 2048, None, 2048, None, 256, None, 256, None, 1, None, 0, None) == -1, "bf16x3 null operands")
ok(lib.vqa_gemm_bf16x3(0, 250, 256, 2048, C.c_void_p(4096), 2048, C.c_void_p(4096), 256, C.c_void_p(4096), 256, None, 1, None, 0,
                       None) == -4, "bf16x3 ragged tile")
ok(lib.vqa_gemm_bf16x3(1, 256, 256, 2048, C.c_void_p(4096), 128, C.c_void_p(4096), 256, C.c_void_p(4096), 256, None, 1, None, 0,
                       None) == -1, "bf16x3 transposed leading dimension")
ok(lib.vqa_gemm_bf16x3(0, 256, 256, 2048, C.c_void_p(4096), 2048, C.c_void_p(4096), 256, C.c_void_p(4096), 256, None, 4, None, 0,
                       None) == -5, "bf16x3 split k without a workspace")
ok(lib.vqa_gemm_bf16x3_set_mode(0) == 0 and lib.vqa_gemm_bf16x3_set_mode(-1) == 0, "bf16x3 mode")
ok(lib.vqa_clock_sample(500.0, 8, 8, None, None) == -1 and lib.vqa_clock_sample(0.5, 8, 8, C.c_void_p(4096), None) == -1 and
   lib.vqa_clock_sample(500.0, 0, 8, C.c_void_p(4096), None) == -1 and lib.vqa_clock_sample(500.0, 8, 65, C.c_void_p(4096), None) == -1 and
   lib.vqa_clock_sample(1e5, 4096, 8, C.c_void_p(4096), None) == -1, "clock sampler arguments")
ok(lib.vqa_gemm_set_gru_config(30) == 0 and lib.vqa_gemm_set_gru_config(19) == -1 and lib.vqa_gemm_set_gru_config(-1) == 0, "gru config ids")

# weight-stationary recurrence: sizes, refusals and switches (no launch: no GPU here, so "supported" is 0 for every shape)
ok(lib.vqa_gru_ws_workspace_bytes(14) == ((3 * 14 + 1) * 8 * 2 * 128 * 256 + 1024) * 4 and lib.vqa_gru_ws_workspace_bytes(-1) == 0, "ws workspace")
ok(lib.vqa_gru_ws_workspace_bytes(1) % 16 == 0, "ws workspace alignment")
for (T, B, H) in ((14, 512, 1024), (14, 513, 1024), (0, 512, 1024), (14, 512, 512), (3, 0, 1024)):
    ok(lib.vqa_gru_ws_supported(T, B, H) == 0 and lib.vqa_gru_ws_bwd_supported(T, B, H) == 0, "ws needs a device %r" % ((T, B, H),))
p4 = C.c_void_p(4096)
ok(lib.vqa_gru_seq_fwd_ws(None, p4, p4, p4, p4, p4, p4, p4, p4, 14, 512, 1024, p4, None) == -1, "ws forward null xp")
ok(lib.vqa_gru_seq_fwd_ws(p4, p4, p4, p4, p4, p4, p4, p4, p4, 14, 512, 1024, None, None) == -1, "ws forward null workspace")
ok(lib.vqa_gru_seq_fwd_ws(p4, p4, p4, p4, p4, p4, p4, p4, p4, 14, 512, 1024, p4, None) == -4, "ws forward without a device")
ok(lib.vqa_gru_seq_bwd_ws(None, None, p4, p4, p4, p4, p4, p4, p4, p4, 14, 512, 1024, p4, None) == -1, "ws backward null dh")
ok(lib.vqa_gru_seq_bwd_ws(p4, None, p4, p4, p4, p4, p4, p4, p4, p4, 14, 512, 1024, p4, None) == -4, "ws backward without a device")
ok(lib.vqa_gru_ws_set_mode(1) == 0 and lib.vqa_gru_ws_set_mode(0) == 0 and lib.vqa_gru_ws_set_mode(-1) == 0, "ws mode")
ok(lib.vqa_gru_ws_set_form(3) == 0 and lib.vqa_gru_ws_set_form(0) == 0 and lib.vqa_gru_ws_set_stamps(None) == 0, "ws tuning switches")
# the step's recurrence form, asked without a step (no device: never weight-stationary)
d = _lib.Dims(B=512, R=4, D=8, H=1024, T=4, W=12, A=8, Vq=16, N_img=4, model_type=0, keep_att=0.8, keep_joint=0.5, inv_global_batch=1 / 512)
live = (C.c_int32 * 4)(512, 300, 7, 0)
for bw in (0, 1):
    ok(lib.vqa_fusion_gru_form(C.byref(d), None, bw) == 2, "gru form without live_rows: chains")
    ok(lib.vqa_fusion_gru_form(C.byref(d), C.cast(live, C.c_void_p), bw) == 1, "gru form with live_rows: live")
ok(lib.vqa_fusion_gru_form(None, None, 0) == -1 and lib.vqa_fusion_gru_form(C.byref(d), None, 2) == -1, "gru form bad arguments")
d.model_type = 12
ok(lib.vqa_fusion_gru_form(C.byref(d), None, 0) == -4, "gru form of the bi-directional encoder")

print("host ABI exercise: %d checks passed on %s" % (checks, _lib.lib_path()))
