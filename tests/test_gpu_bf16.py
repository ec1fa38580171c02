"""The opt-in bf16 mixed-precision mode on the GPU: vqa_gemm_bf16 (ops.gemm_bf16; split-k workspace from
vqa_gemm_bf16_workspace_floats) against the float64 reference of the op, and FusionEngine(precision="bf16")
(VQA_FLAG_BF16_GEMM) against the float64 restatement of the step with rounded routed products (tests/bf16_ref.py).
The tolerances live beside the references; tests/test_bf16_ref.py holds them to a tenth of what a wrong kernel or a
step that ignored the flag would show."""
import argparse
import ctypes as C
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import vqa_oracle as O
from tests import bf16_ref as R
from tests.gpu_util import dev, dev_batch, make_case, make_engine

pytestmark = pytest.mark.gpu

# worst max |got - ref| / (|A^||B^|) measured on the MI355X over every case below: R.OP_TOL_MEASURED;
# tolerance R.OP_TOL = 3 x that (profiles/r8_bf16_bench.txt)
OP_TOL = R.OP_TOL


def _ops():
    from vqa_transfer_externaldata_amd import ops
    return ops


def _check(got, A, B, tA, tB, bias, add, what):
    ref = R.gemm_ref(A, B, tA, tB, bias, add)
    sc = R.gemm_scale(A, B, tA, tB)
    assert torch.isfinite(got).all(), what
    ratio = float(((got.double() - ref).abs() / sc.clamp_min(1e-300)).max())
    print("%s: ratio %.3e" % (what, ratio))
    assert ((got.double() - ref).abs() <= OP_TOL * sc).all(), (what, ratio)
    return ratio


OP_CASES = [(lay, M, N, K) for (M, N, K) in R.SMALL_SHAPES for lay in ("NN", "TN", "NT")] + list(R.STEP_SHAPES)


@pytest.mark.parametrize("lay,M,N,K", OP_CASES, ids=["%s-%dx%dx%d" % c for c in OP_CASES])
def test_gemm_bf16_matches_the_float64_reference(lay, M, N, K):
    ops = _ops()
    for seed in R.OP_SEEDS:
        A, B, bias, add, tA, tB = R.op_case(lay, M, N, K, seed, device="cuda", bias=True, add=True)
        for split in (1, 0, 3):
            for use_bias, use_add in ((False, False), (True, True)) if split != 3 else ((True, False), (False, True)):
                bv, ad = (bias if use_bias else None), (add if use_add else None)
                out = torch.full((M, N), float("nan"), device="cuda")               # poisoned: every element must be written
                got = ops.gemm_bf16(A, B, transA=tA, transB=tB, bias=bv, add=ad, split_k=split, out=out)
                assert got is out
                _check(got, A, B, tA, tB, bv, ad, "%s %dx%dx%d seed %d split %d bias %d add %d" % (lay, M, N, K, seed, split, use_bias, use_add))
                again = ops.gemm_bf16(A, B, transA=tA, transB=tB, bias=bv, add=ad, split_k=split)
                assert torch.equal(again, got), "two calls with the same inputs differ"


@pytest.mark.parametrize("lay", ["NN", "TN", "NT"])
def test_gemm_bf16_strided_output_unaligned_operands_and_in_place_addend(lay):
    ops = _ops()
    M, N, K = 250, 130, 77
    A, B, bias, add, tA, tB = R.op_case(lay, M, N, K, 5, device="cuda", bias=True, add=True)
    # strided out: a column window of a wider, poisoned buffer; the columns beside it stay untouched
    wide = torch.full((M, N + 37), float("nan"), device="cuda")
    out = wide[:, 5:5 + N]
    for split in (1, 4):
        wide.fill_(float("nan"))
        ops.gemm_bf16(A, B, transA=tA, transB=tB, bias=bias, split_k=split, out=out)
        _check(out, A, B, tA, tB, bias, None, "%s strided out split %d" % (lay, split))
        assert torch.isnan(wide[:, :5]).all() and torch.isnan(wide[:, 5 + N:]).all()
    # operands that are windows of wider buffers at odd offsets: leading dimensions / bases off the 16-byte grid
    Aw = torch.full((A.shape[0], A.shape[1] + 3), float("nan"), device="cuda")
    Bw = torch.full((B.shape[0], B.shape[1] + 5), float("nan"), device="cuda")
    Aw[:, 1:1 + A.shape[1]] = A
    Bw[:, 3:3 + B.shape[1]] = B
    Av, Bv = Aw[:, 1:1 + A.shape[1]], Bw[:, 3:3 + B.shape[1]]
    got = ops.gemm_bf16(Av, Bv, transA=tA, transB=tB, bias=bias, add=add)
    _check(got, A, B, tA, tB, bias, add, "%s unaligned operands" % lay)
    assert torch.equal(got, ops.gemm_bf16(A, B, transA=tA, transB=tB, bias=bias, add=add))      # the slower path: same bits
    # addend = the output itself (dx accumulation of the step)
    acc = add.clone()
    ops.gemm_bf16(A, B, transA=tA, transB=tB, add=acc, out=acc)
    _check(acc, A, B, tA, tB, None, add, "%s in-place addend" % lay)


@pytest.mark.parametrize("lay,M,N,K,split", [("NN", 130, 70, 96, 1), ("TN", 64, 200, 160, 4), ("NT", 257, 33, 100, 0)])
def test_gemm_bf16_is_exact_on_small_integers(lay, M, N, K, split):
    """operands already bf16-representable (integers in [-8, 8]) and |sums| < 2^24: every product and partial sum is
    exact in f32, so is the result, in every summation order"""
    ops = _ops()
    g = torch.Generator().manual_seed(9)
    tA, tB = lay == "TN", lay == "NT"
    A = torch.randint(-8, 9, (K, M) if tA else (M, K), generator=g).float().cuda()
    B = torch.randint(-8, 9, (N, K) if tB else (K, N), generator=g).float().cuda()
    bias = torch.randint(-100, 100, (N,), generator=g).float().cuda()
    add = torch.randint(-100, 100, (M, N), generator=g).float().cuda()
    got = ops.gemm_bf16(A, B, transA=tA, transB=tB, bias=bias, add=add, split_k=split)
    want = (A.t() if tA else A).double() @ (B.t() if tB else B).double() + bias.double() + add.double()
    assert torch.equal(got.double(), want)


def test_gemm_bf16_argument_checks_launch_nothing():
    from vqa_transfer_externaldata_amd import _lib
    lib = _lib.load()
    A = torch.ones(256, 2048, device="cuda")
    B = torch.ones(2048, 256, device="cuda")
    out = torch.full((256, 256), 7.0, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda *a: lib.vqa_gemm_bf16(*a)
    assert call(0, 0, 256, 256, 2048, None, 2048, p(B), 256, p(out), 256, None, None, 0, 1, None, 0, 0, st) == -1       # null A
    assert call(0, 0, 256, 256, 2048, p(A), 2048, None, 256, p(out), 256, None, None, 0, 1, None, 0, 0, st) == -1       # null B
    assert call(0, 0, 256, 256, 2048, p(A), 2048, p(B), 256, None, 256, None, None, 0, 1, None, 0, 0, st) == -1         # null C
    assert call(0, 0, 256, 256, 2048, p(A), 2047, p(B), 256, p(out), 256, None, None, 0, 1, None, 0, 0, st) == -1       # lda < K
    assert call(0, 0, 256, 256, 2048, p(A), 2048, p(B), 255, p(out), 256, None, None, 0, 1, None, 0, 0, st) == -1       # ldb < N
    assert call(0, 0, 256, 256, 2048, p(A), 2048, p(B), 256, p(out), 255, None, None, 0, 1, None, 0, 0, st) == -1       # ldc < N
    assert call(1, 0, 256, 256, 2048, p(A), 255, p(B), 256, p(out), 256, None, None, 0, 1, None, 0, 0, st) == -1        # transA: lda < M
    assert call(0, 0, 0, 256, 2048, p(A), 2048, p(B), 256, p(out), 256, None, None, 0, 1, None, 0, 0, st) == -1         # M < 1
    assert call(1, 1, 256, 256, 2048, p(A), 2048, p(B), 2048, p(out), 256, None, None, 0, 1, None, 0, 0, st) == -4      # both transposed
    assert lib.vqa_gemm_bf16_workspace_floats(256, 256, 2048, 4) == 4 * 256 * 256
    assert lib.vqa_gemm_bf16_workspace_floats(256, 256, 2048, 1) == 0
    assert call(0, 0, 256, 256, 2048, p(A), 2048, p(B), 256, p(out), 256, None, None, 0, 4, None, 0, 0, st) == -5       # split k, no workspace
    ws = torch.zeros(4 * 256 * 256 - 1, device="cuda")
    assert call(0, 0, 256, 256, 2048, p(A), 2048, p(B), 256, p(out), 256, None, None, 0, 4, p(ws), ws.numel(), 0, st) == -5   # too small
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ws == 0).all()                                     # nothing was launched


# ---------------------------------------------------------------------------------------------------------- the model
def _run(eng, batch, masks, lr=None):
    ka, kj = dev(masks["att"].astype(np.uint8)), dev(masks["joint"].astype(np.uint8))
    eng.forward(dev_batch(batch), ka, kj, want_dz=True)
    eng.backward()
    if lr is not None:
        eng.optimizer_step(lr)
    torch.cuda.synchronize()


@pytest.mark.parametrize("model_type", R.MODEL_TYPES)
@pytest.mark.parametrize("case", R.MODEL_CASES, ids=[c[0] for c in R.MODEL_CASES])
def test_bf16_step_matches_the_rounded_float64_reference(model_type, case):
    """Loss, logits, the 13 report scalars and every trainable gradient of FusionEngine(precision="bf16") against
    tests/bf16_ref.py (tolerances and their derivation: there).  Every figure is printed before it is asserted.
    The reference rounds the step's own routed operands (its `witness` mode): each of them must lie within
    R.WITNESS_TOL of the reference's own value, and then both sides round the same numbers.  Without that, activations
    near a bf16 rounding boundary round differently on the two sides and the flips feed on each other: measured on the
    MI355X, logits 2.9e-3 and gradients up to 3.6e-3 of the tensor's max apart at D = 2048, H = 1024, 5.3e-4 at the medium
    size (profiles/r8_bf16_bench.txt) -- 10 - 30 % of all that separates the flag on from the flag off."""
    name, dims, B, Rg, T, N = case
    p, table, nbox, batch, am, masks = make_case(R.MODEL_SEED, model_type, B, Rg, T, N, dims)
    eng = make_engine(model_type, p, table, nbox, am, B, Rg, T, dims, precision="bf16")
    assert eng.precision == "bf16"
    _run(eng, batch, masks)
    pp = {k: v for k, v in p.items() if not O.is_const(k)}
    D, H, A = dims["D"], dims["H"], dims["A"]
    g = lambda n, *shape: eng.tensor(n).view(*shape).cpu().numpy()
    witness = {"v_linear_v": {"x": g("V_ft", B, Rg, D), "d": g("d_pre_v", B, Rg, H)},
               "q_linear_v": {"x": g("condition", B, H), "d": g("d_pre_qv", B, H)},
               "pooled_linear_l": {"x": g("pooled_V_ft", B, D), "d": g("d_pre_pl", B, H)},
               "q_linear_l": {"x": g("condition", B, H), "d": g("d_pre_ll", B, H)},
               "joint_fc": {"x": g("joint_in", B, H), "d": g("d_pre_j", B, 2 * H)},
               "head": {"x": g("joint", B, 2 * H), "d": g("dlogit", B, A)}}
    loss, mid, grads, dx, report = R.loss_and_grads(pp, batch, table, nbox, am, masks, model_type, rounding=True, witness=witness)
    fails = []

    def hold(what, err, tol):
        print("%-58s err %.3e  tol %.3e" % (what, err, tol))
        if not err <= tol:
            fails.append((what, err, tol))

    for k in R.ROUTED:
        for side in ("x", "d"):
            hold("witness %s %s" % (k, side), witness[k]["log"][side], R.WITNESS_TOL)
    z = eng.tensor("logit").view(B, dims["A"]).cpu().numpy().astype(np.float64)
    hold("logit (abs)", np.abs(z - mid["logit"]).max(), R.LOGIT_TOL)
    rep = eng.report()
    hold("loss", abs(float(eng.loss()) - loss), R.LOSS_TOL * max(1.0, abs(loss)))
    for k in O.REPORT_KEYS:
        tol = R.LOSS_TOL if k in ("answer_train_loss", "answer_report_loss") else R.REPORT_TOL
        hold("report " + k, abs(rep[k] - report[k]), tol * max(1.0, abs(report[k])))
    np.testing.assert_array_equal(eng.tensor("pred").cpu().numpy(), mid["pred"])
    for n in eng.train_names:
        if n.endswith("score/fc/biases"):
            assert abs(float(eng.grads[n][0])) <= 1e-5            # analytically zero (softmax shift invariance)
            continue
        hold("grad " + n, R.grad_distance(eng.grads[n].cpu().numpy(), grads[n]), R.GRAD_TOL)
    hold("grad dx_embed", R.grad_distance(eng.tensor("dx_embed").view(T, B, dims["W"]).transpose(0, 1).cpu().numpy(), dx), R.GRAD_TOL)
    assert not fails, fails


@pytest.mark.parametrize("mt", R.MODEL_TYPES)
@pytest.mark.parametrize("case", R.MODEL_CASES[1:], ids=[c[0] for c in R.MODEL_CASES[1:]])
def test_every_routed_site_rounds_and_the_encoder_does_not(case, mt):
    """Site by site on the step's OWN activations (no rounding flips between the two sides, so the op tolerance applies):
    each routed product of the step -- forward pre-activation, dW where the layer trains, dx, the two dx products that
    meet in d(condition) -- equals round(x) round(W) of the tensors the step itself read, to R.OP_TOL (|x^||W^|), and is
    at least 100 x R.OP_TOL from the product of the unrounded operands; the x-projection of the GRU equals the UNROUNDED
    product."""
    name, dims, B, Rg, T, N = case
    p, table, nbox, batch, am, masks = make_case(R.MODEL_SEED, mt, B, Rg, T, N, dims)
    eng = make_engine(mt, p, table, nbox, am, B, Rg, T, dims, precision="bf16")
    # forward + phase 1 of backward only: d(condition) as the dense layers leave it, before the recurrence's backward reads it
    ka, kj = dev(masks["att"].astype(np.uint8)), dev(masks["joint"].astype(np.uint8))
    eng.forward(dev_batch(batch), ka, kj, want_dz=True)
    eng.grad_flat[:eng.embed_floats].zero_()
    eng._backward_phases(1)
    torch.cuda.synchronize()
    sc, D, H, A, W = eng.sc, dims["D"], dims["H"], dims["A"], dims["W"]
    t = lambda n, *shape: eng.tensor(n).view(*shape)
    sites = [("v_linear_v", t("V_ft", B * Rg, D), "pre_v", "d_pre_v", H, None), ("q_linear_v", t("condition", B, H), "pre_qv", "d_pre_qv", H, None),
             ("pooled_linear_l", t("pooled_V_ft", B, D), "pre_pl", "d_pre_pl", H, "d_pooled"),
             ("q_linear_l", t("condition", B, H), "pre_ll", "d_pre_ll", H, None),
             ("joint_fc", t("joint_in", B, H), "pre_j", "d_pre_j", 2 * H, "d_joint_in"), ("head", t("joint", B, 2 * H), "logit", "dlogit", A, "d_joint")]
    worst = 0.0
    for key, x, pre, dpre, n_out, dx in sites:
        Wt, b = eng.params[sc[key] + "/fc/weights"], eng.params[sc[key] + "/fc/biases"]
        d = t(dpre, x.shape[0], n_out)
        checks = [("fwd", t(pre, x.shape[0], n_out), (x, Wt, False, False, b))]
        if sc[key] + "/fc/weights" in eng.grads:                   # frozen layers of vlmap_answer have no dW
            checks.append(("dW", eng.grads[sc[key] + "/fc/weights"], (x, d, True, False, None)))
        if dx is not None:
            checks.append(("dx", t(dx, *x.shape), (d, Wt, False, True, None)))
        for what, got, (a, bb, tA, tB, bias) in checks:
            scale = R.gemm_scale(a, bb, tA, tB) + (bias.double().abs() if bias is not None else 0)    # the bias add rounds too
            r = float(((got.double() - R.gemm_ref(a, bb, tA, tB, bias)).abs() / scale.clamp_min(1e-300)).max())
            worst = max(worst, r)
            print("%-16s %-3s ratio %.3e" % (key, what, r))
            assert r <= R.OP_TOL, (key, what, r)
            # the same figure against the product of the UNROUNDED operands: three orders of magnitude away
            ref = (a.t() if tA else a).double() @ (bb.t() if tB else bb).double() + (bias.double() if bias is not None else 0)
            far = float(((got.double() - ref).abs() / scale.clamp_min(1e-300)).max())
            assert far >= 100 * R.OP_TOL, (key, what, far)
    assert mt != "standard" or all(sc[k] + "/fc/weights" in eng.grads for k in R.ROUTED)
    # d(condition) = d_pre_ll W_ll^T, then + d_pre_qv W_qv^T added in f32 by the second product's addend
    dll, dqv = t("d_pre_ll", B, H), t("d_pre_qv", B, H)
    Wll, Wqv = eng.params[sc["q_linear_l"] + "/fc/weights"], eng.params[sc["q_linear_v"] + "/fc/weights"]
    ref = R.gemm_ref(dll, Wll, False, True) + R.gemm_ref(dqv, Wqv, False, True)
    scale = R.gemm_scale(dll, Wll, False, True) + R.gemm_scale(dqv, Wqv, False, True)
    got = t("d_h0", B, H).double()
    r = float(((got - ref).abs() / scale.clamp_min(1e-300)).max())
    far = float(((got - (dll.double() @ Wll.double().t() + dqv.double() @ Wqv.double().t())).abs() / scale.clamp_min(1e-300)).max())
    print("q_linear_l + q_linear_v dx (d condition) ratio %.3e, against the unrounded products %.3e" % (r, far))
    assert r <= R.OP_TOL and far >= 100 * R.OP_TOL, (r, far)
    # unrouted: xp = x_tm[:, :W] wx_cat + bx_cat on the f32 MFMA
    Wp = (W + 1 + 3) // 4 * 4
    x, wx, bx = t("x_tm", T * B, Wp)[:, :W], t("wx_cat", W, 3 * H), t("bx_cat", 3 * H)
    ref = x.double() @ wx.double() + bx.double()
    r = float(((t("xp", T * B, 3 * H).double() - ref).abs() / (x.double().abs() @ wx.double().abs() + bx.double().abs())).max())
    print("gru x-projection against the unrounded product: ratio %.3e" % r)
    assert r <= R.OP_TOL, r


@pytest.mark.parametrize("model_type", R.MODEL_TYPES)
def test_precision_f32_is_bitwise_the_engine_without_the_argument(model_type):
    dims, B, Rg, T, N = R.MED, 32, 36, 14, 64
    p, table, nbox, batch, am, masks = make_case(31, model_type, B, Rg, T, N, dims)
    res = []
    for kw in ({}, {"precision": "f32"}, {"precision": "bf16"}):
        eng = make_engine(model_type, p, table, nbox, am, B, Rg, T, dims, deterministic=True, **kw)
        for _ in range(2):
            _run(eng, batch, masks, lr=1e-3)
        res.append((eng.precision, float(eng.loss()), eng.grad_flat.clone(), eng.train_flat.clone()))
    (p0, l0, g0, t0), (p1, l1, g1, t1), (p2, l2, g2, t2) = res
    assert (p0, p1, p2) == ("f32", "f32", "bf16")
    assert l0 == l1 and torch.equal(g0, g1) and torch.equal(t0, t1)
    assert not torch.equal(g0, g2)                                # and the flag does change the products


def test_refusals():
    from vqa_transfer_externaldata_amd import _lib
    dims, B, Rg, T, N = R.SMALL, 5, 6, 7, 9
    for mt in ("standard_word2vec", "standard_testmask", "vlmap_answer_vqa_all2", "vlmap_answer_noc", "vlmap_answer_adapt"):
        p, table, nbox, batch, am, masks = make_case(3, mt, B, Rg, T, N, dims)
        with pytest.raises(ValueError, match="bf16"):
            make_engine(mt, p, table, nbox, am, B, Rg, T, dims, precision="bf16")
    p, table, nbox, batch, am, masks = make_case(3, "vlmap_answer", B, Rg, T, N, dims)
    with pytest.raises(ValueError, match="fused_gather"):
        make_engine("vlmap_answer", p, table, nbox, am, B, Rg, T, dims, precision="bf16", fused_gather=True)
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError, match="precision"):
            make_engine("vlmap_answer", p, table, nbox, am, B, Rg, T, dims, precision=bad)
    # the entry points refuse the same combinations with VQA_ERR_ARG (no half-routed step)
    lib = _lib.load()
    eng = make_engine("vlmap_answer", p, table, nbox, am, B, Rg, T, dims, precision="bf16")
    assert eng.dims.flags & _lib.FLAG_BF16_GEMM == 8
    ka, kj = dev(masks["att"].astype(np.uint8)), dev(masks["joint"].astype(np.uint8))
    eng.forward(dev_batch(batch), ka, kj)
    for model_type, flags in ((2, 8), (5, 8), (9, 8), (12, 8), (0, 8 | 2)):
        d = _lib.Dims.from_buffer_copy(eng.dims)
        d.model_type, d.flags = model_type, flags
        assert lib.vqa_fusion_workspace_bytes(C.byref(d)) == -1
        args = (C.byref(d), C.byref(eng._p_struct), C.byref(eng._bs), C.c_void_p(eng.workspace.data_ptr()), eng.workspace.numel())
        assert lib.vqa_fusion_forward(*args, 1, eng._stream()) == -1
        assert lib.vqa_fusion_backward_phases(C.byref(d), C.byref(eng._p_struct), C.byref(eng._g_struct), C.byref(eng._bs),
                                              C.c_void_p(eng.workspace.data_ptr()), eng.workspace.numel(), None, 15,
                                              eng._stream()) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- trainer
def _trainer_config(tmp_path, sub, precision):
    from vqa_transfer_externaldata_amd import trainer
    c = trainer.parse_config(["--batch_size", "32", "--max_train_iter", "12", "--train_average_iter", "4",
                              "--val_average_iter", "2", "--validation_step", "6", "--checkpoint_step", "6",
                              "--heavy_summary_step", "6", "--model_type", "standard", "--learning_rate", "0.002",
                              "--precision", precision])
    Vq, A = 60, 40
    c.vocab = {"vocab": ["w%d" % i for i in range(Vq)], "dict": {"w%d" % i: i for i in range(Vq)}}
    c.answer_dict = {"vocab": ["a%d" % i for i in range(A)], "dict": {"a%d" % i: i for i in range(A)},
                     "num_train_answer": 30, "is_object": [i % 2 for i in range(A)],
                     "is_attribute": [1 - i % 2 for i in range(A)]}
    c.synthetic = 1
    c.train_dir = str(tmp_path / sub)
    c.tf_record_dir = str(tmp_path / "data")
    return c, Vq, A


def _features(n_img=24, Rg=36, D=64):
    rng = np.random.default_rng(0)
    return {"features": np.maximum(rng.standard_normal((n_img, Rg, D)), 0).astype(np.float32),
            "spatials": np.zeros((n_img, Rg, 6), np.float32), "normal_boxes": np.zeros((n_img, Rg, 4), np.float32),
            "num_boxes": np.full(n_img, Rg, np.int32), "max_box_num": Rg, "vfeat_dim": D}


def test_trainer_bf16_learns_and_its_checkpoint_loads_in_an_f32_evaler(tmp_path):
    from vqa_transfer_externaldata_amd import evaler, input_ops_vqa as io, trainer
    losses = {}
    for precision in ("bf16", "f32"):
        c, Vq, A = _trainer_config(tmp_path, "run_" + precision, precision)
        ds = {"train": io.synthetic_split(96, 24, Vq, A, seed=1), "val": io.synthetic_split(40, 24, Vq, A, seed=2),
              "testval": io.synthetic_split(40, 24, Vq, A, seed=3)}
        t = trainer.Trainer(c, datasets=ds, image_features=_features())
        assert t.model.engine.precision == precision
        val_loss = lambda: float(np.mean([t.run_val_step(False, "val")[2] for _ in range(4)]))   # dropout off, same split
        loss0 = val_loss()
        t.run_train_step(True)
        t.train()
        loss1 = val_loss()
        losses[precision] = (loss0, loss1)
        if precision == "bf16":
            assert np.isfinite(loss0) and np.isfinite(loss1) and loss1 < loss0
            assert all(torch.isfinite(v).all() for v in t.model.variables().values())
            ckpt = os.path.join(c.train_dir, "model-8")
            assert os.path.exists(ckpt)
            sd = torch.load(ckpt)
            assert all(v.dtype in (torch.float32, torch.int64) for v in sd.values())           # f32 parameters and Adam slots
            ec = argparse.Namespace(**vars(c))
            ec.checkpoint, ec.split, ec.max_iter, ec.dump_heavy_output, ec.precision = ckpt, "testval", -1, False, "f32"
            ev = evaler.Evaler(ec, image_features=_features(), data=ds["testval"])
            assert ev.model.engine.precision == "f32"
            ev.eval()
            saved = pickle.load(open(ev.save_pkl, "rb"))
            assert len(saved["qid2result"]) == 40 and np.isfinite(saved["avg_eval_report"]["answer_report_loss"])
    print("validation loss before / after 13 train steps: bf16 %.5f / %.5f, f32 %.5f / %.5f (for the record)"
          % (losses["bf16"] + losses["f32"]))


# ---------------------------------------------------------------------------------------------------------- data parallel
DP_DIMS = dict(Vq=500, W=300, D=256, H=128, A=300)
DP_B, DP_R, DP_T, DP_N = 7, 36, 14, 20


def _dp_steps(eng, batch, masks, reducer):
    ka, kj = dev(masks["att"].astype(np.uint8)), dev(masks["joint"].astype(np.uint8))
    db = dev_batch(batch)
    first = None
    for _ in range(2):
        eng.train_step(db, ka, kj, 1e-3, allreduce=reducer)
        if first is None:
            torch.cuda.synchronize()
            first = eng.grad_flat.cpu().numpy().copy()
    torch.cuda.synchronize()
    return first, eng.train_flat.cpu().numpy().copy()


def _dp_worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vqa_transfer_externaldata_amd import dp
    p, table, nbox, batch, am, masks = make_case(77, "vlmap_answer", DP_B, DP_R, DP_T, DP_N, DP_DIMS)
    shard, n_global = dp.shard_batch(batch, rank, world)
    lo, hi = dp.shard_bounds(n_global, rank, world)
    m = {k: v[lo:hi] for k, v in masks.items()}
    eng = make_engine("vlmap_answer", p, table, nbox, am, hi - lo, DP_R, DP_T, DP_DIMS, global_batch=n_global, precision="bf16")
    g1, params = _dp_steps(eng, shard, m, dp.BucketedAllReduce())
    if rank == 0:
        np.savez(out_path, g1=g1, params=params)
    dist.barrier()
    dist.destroy_process_group()


def test_bf16_two_ranks_equal_one_process_full_batch(tmp_path):
    """tests/test_gpu_dp.py's world-2 case with precision="bf16" on both sides and that file's tolerances: gradients
    are f32 on the wire, the flag needs no collective"""
    world = 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out_path = str(tmp_path / "rank0.npz")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, out_path)) for r in range(world)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0
    got = np.load(out_path)
    p, table, nbox, batch, am, masks = make_case(77, "vlmap_answer", DP_B, DP_R, DP_T, DP_N, DP_DIMS)
    eng = make_engine("vlmap_answer", p, table, nbox, am, DP_B, DP_R, DP_T, DP_DIMS, precision="bf16")
    g1, params = _dp_steps(eng, batch, masks, None)
    n = eng.n_train
    for name, (off, cnt) in eng._train_tab.items():
        if name.endswith("score/fc/biases"):
            continue                                  # analytically zero
        a, b = got["g1"][off:off + cnt], g1[off:off + cnt]
        sc = max(np.abs(b).max(), 1e-12)
        assert np.abs(a - b).max() <= 2e-5 * sc + 1e-10, (name, np.abs(a - b).max(), sc)
    assert abs(got["g1"][n] - g1[n]) <= 1e-5 * g1[n]
    d = np.abs(got["params"] - params)
    assert d.max() <= 2.5e-4, d.max()
    assert np.mean(d > 2e-5) < 0.01, np.mean(d > 2e-5)
