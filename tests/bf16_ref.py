"""Float64 reference of the bf16 mixed-precision mode (include/vqa_hot.h, VQA_FLAG_BF16_GEMM).

TEST INFRASTRUCTURE ONLY.  Two layers:

  * the op: gemm_ref = round(A) @ round(B) (+ bias) (+ addend) in float64, round = nearest-even rounding to bf16;
  * the step of the accepted model types (vlmap_answer, standard): a torch restatement in float64 in which every ROUTED
    product (forward, dW, dx of v_linear_v, q_linear_v, pooled_linear_l, q_linear_l, joint_fc and the answer head) goes
    through one autograd function that rounds both operands of each of its three products, and everything else -- the
    question encoder, LayerNorm, attention, loss -- is plain float64.  With `rounding=False` it is oracle/torch_ref.py
    (tests/test_bf16_ref.py holds it to that).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vqa_oracle as O

MODEL_TYPES = ("vlmap_answer", "standard")
# layer -> scope key of the routed dense layers, in the order of the header's list
ROUTED = ("v_linear_v", "q_linear_v", "pooled_linear_l", "q_linear_l", "joint_fc", "head")
UNROUTED = ("gru_gates", "gru_cand")


def round_bf16(x):
    """x rounded to the nearest bf16 (ties to even), returned in x's dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


def truncate_bf16(x):
    """the WRONG conversion (discrimination tests): the low 16 bits of the float32 pattern dropped"""
    bits = x.float().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).to(x.dtype)


def _op(X, trans):
    return X.t() if trans else X


def gemm_ref(A, B, transA=False, transB=False, bias=None, add=None, round_a=round_bf16, round_b=round_bf16):
    """float64 [M,N] on the operands' device: round(op(A)) @ round(op(B)) + bias + add (operands float32 tensors)"""
    a = round_a(_op(A, transA).detach().float()).double()
    b = round_b(_op(B, transB).detach().float()).double()
    c = a @ b
    if bias is not None:
        c = c + bias.detach().double()
    if add is not None:
        c = c + add.detach().double()
    return c


def gemm_scale(A, B, transA=False, transB=False):
    """(|round A| |round B|)_ij in float64: the per-element yardstick of the op criterion"""
    a = round_bf16(_op(A, transA).detach().float()).double().abs()
    b = round_bf16(_op(B, transB).detach().float()).double().abs()
    return a @ b


def op_case(layout, M, N, K, seed, device="cpu", bias=False, add=False):
    """the normal random operands of the op tests, generated on the CPU from the seed: (A, B, bias, add, transA, transB)
    with A / B stored the way the layout reads them (NN: [M,K] [K,N]; TN: [K,M] [K,N]; NT: [M,K] [N,K])"""
    g = torch.Generator().manual_seed(seed)
    tA, tB = layout == "TN", layout == "NT"
    A = torch.randn((K, M) if tA else (M, K), generator=g)
    B = torch.randn((N, K) if tB else (K, N), generator=g)
    bv = torch.randn(N, generator=g) if bias else None
    ad = torch.randn(M, N, generator=g) if add else None
    mv = lambda t: t.to(device) if t is not None else None
    return mv(A), mv(B), mv(bv), mv(ad), tA, tB


def op_ratio(got, A, B, transA=False, transB=False, bias=None, add=None):
    """max_ij |got - ref|_ij / (|round A| |round B|)_ij  -- the figure the op tolerance bounds"""
    ref = gemm_ref(A, B, transA, transB, bias, add)
    sc = gemm_scale(A, B, transA, transB)
    return float(((got.double() - ref).abs() / sc.clamp_min(1e-300)).max())


# shapes of the op tests: the four of the discrimination test, then the step's own (layout, M, N, K)
SMALL_SHAPES = [(256, 256, 2048), (512, 1024, 1024), (128, 384, 300), (250, 130, 77)]
STEP_SHAPES = [("NN", 18432, 1024, 2048), ("TN", 2048, 1024, 18432), ("NN", 512, 3000, 2048), ("NT", 512, 2048, 3000),
               ("NN", 1, 1, 1)]
OP_SEEDS = (0, 1)


# ---- tolerances of the GPU tests (tests/test_gpu_bf16.py); tests/test_bf16_ref.py holds each to a tenth of what a wrong
# implementation would show, computed on the CPU from the references alone.
# Op: |got - ref| <= OP_TOL (|A^||B^|)_ij.  Worst ratio measured on the MI355X over every case of the op test
# (profiles/r8_bf16_bench.txt): OP_TOL_MEASURED; OP_TOL = 3 x that, the margin for another legal f32 summation order.
OP_TOL_MEASURED = 2.644e-7      # the 1 x 1 x 1 case with bias and addend: one f32 rounding of a sum larger than |a b|
OP_TOL = 3 * OP_TOL_MEASURED
# Model, against this file's float64 step.  Gradients: max |got - ref| <= GRAD_TOL max |ref| per tensor, logits LOGIT_TOL
# absolute, the two losses LOSS_TOL max(1, |loss|), the other report scalars REPORT_TOL max(1, |x|) (means of 0 / 1 scores:
# exact unless an argmax changes).  tests/test_gpu_fusion.py holds the f32 step to 5e-4 / 1e-3 / 1e-4 against the float64
# oracle; a step that ignored the flag sits 1.1e-3 (gradients), 9.5e-3 (logits) and 3.0e-5 (loss) from this reference on the
# cases below, so GRAD_TOL, LOGIT_TOL and LOSS_TOL are at most a tenth of that.
# Rounding flips: an activation within f32 error of a bf16 rounding boundary legally rounds either way, and a difference d
# between the two sides comes out of a rounding as ~ sqrt(d 2^-8); measured without a witness (profiles/r8_bf16_bench.txt)
# the two sides then differ by 10 - 30 % of the rounding noise itself at D = 2048, H = 1024 (gradients up to 3.6e-3, logits
# 2.9e-3), which no bound that still tells the flag on from the flag off can cover.  So the GPU test hands the reference
# the step's own operands as witnesses (_Routed): the reference rounds THOSE, after checking each is within WITNESS_TOL
# (max-normalised; the 2e-4 tests/test_gpu_fusion.py allows a mid result) of its own value.
# What that leaves: the x 10 margin of tests/test_bf16_ref.py is argued from the UNWITNESSED distance between the rounded
# and the unrounded reference; the witnessed comparison itself is a layer-by-layer check with WITNESS_TOL of slack per
# operand, in which a step that ignored the flag would stand out by one layer's rounding only.  What tells the flag on
# from the flag off product by product is test_every_routed_site_rounds_and_the_encoder_does_not (both model types, every
# forward / dW / dx site at OP_TOL, each at least 100 x OP_TOL from the product of the unrounded operands).
GRAD_TOL = 1e-4
LOGIT_TOL = 5e-4
LOSS_TOL = 2.5e-6
REPORT_TOL = 1e-4
WITNESS_TOL = 2e-4
SMALL = dict(Vq=30, W=12, D=24, H=16, A=21)
MED = dict(Vq=500, W=300, D=256, H=128, A=300)
FULL = dict(Vq=2000, W=300, D=2048, H=1024, A=3000)
# (name, dims, B, R, T, N_img) of the model parity / discrimination cases
MODEL_CASES = [("small", SMALL, 5, 6, 7, 9), ("med", MED, 32, 36, 14, 64), ("full_dims", FULL, 8, 36, 14, 24)]
MODEL_SEED = 21


def grad_distance(got, want):
    """max |got - want| / max |want|: the normalised distance of a gradient tensor"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


class _Routed(torch.autograd.Function):
    """y = r(x) r(W); dW = r(x)^T r(dy); dx = r(dy) r(W)^T  with r = round_bf16 (or the identity).
    wit (optional): {"x": the step's own f32 left operand, "d": its own f32 d_pre, "log": dict}.  A computed activation
    that sits within f32 error of a bf16 rounding boundary may legally round either way, and this float64 restatement
    cannot know which way the f32 step went; with a witness it rounds the step's value instead of its own -- after
    recording how far that value is from its own (the caller bounds it by WITNESS_TOL) -- so both sides round the same
    numbers and everything downstream is comparable at the f32 tolerances.  Weights are inputs: never witnessed."""

    @staticmethod
    def forward(ctx, x, W, rounding, wit):
        r = round_bf16 if rounding else (lambda t: t)
        x2 = x.reshape(-1, x.shape[-1])
        if wit is not None:
            xw = wit["x"].reshape(x2.shape)
            wit["log"]["x"] = float((xw - x2).abs().max() / x2.abs().max().clamp_min(1e-300))
            x2 = xw
        xr = r(x2)
        ctx.save_for_backward(xr, W)
        ctx.rounding, ctx.wit, ctx.xshape = rounding, wit, x.shape
        return xr.matmul(r(W)).reshape(x.shape[:-1] + (W.shape[1],))

    @staticmethod
    def backward(ctx, dy):
        xr, W = ctx.saved_tensors
        r = round_bf16 if ctx.rounding else (lambda t: t)
        d2 = dy.reshape(-1, dy.shape[-1])
        if ctx.wit is not None:
            dw = ctx.wit["d"].reshape(d2.shape)
            ctx.wit["log"]["d"] = float((dw - d2).abs().max() / d2.abs().max().clamp_min(1e-300))
            d2 = dw
        dW = xr.t().matmul(r(d2))
        dx = r(d2).matmul(r(W).t()).reshape(ctx.xshape)
        return dx, dW, None, None


def _fc(x, P, scope, rounding, wit=None):
    pre = _Routed.apply(x, P[scope + "/fc/weights"], rounding, wit) + P[scope + "/fc/biases"]
    pre.retain_grad()
    P.setdefault("_tape", {})[scope] = (x, pre)       # left operand and pre-activation of every routed layer
    return pre


def _fc_ln_relu(x, P, scope, rounding, wit=None):
    pre = _fc(x, P, scope, rounding, wit)
    dims = tuple(range(1, pre.dim()))
    mu = pre.mean(dim=dims, keepdim=True)
    var = ((pre - mu) ** 2).mean(dim=dims, keepdim=True)
    return torch.relu((pre - mu) / torch.sqrt(var + O.LN_EPS) * P[scope + "/LayerNorm/gamma"] + P[scope + "/LayerNorm/beta"])


def _gru(x, lens, Wg, bg, Wc, bc):
    """GRUCell over the padded sequence, plain float64 (unrouted)"""
    B, T, W = x.shape
    H = Wc.shape[1]
    h = x.new_zeros(B, H)
    for t in range(T):
        xt = x[:, t]
        g = torch.sigmoid(xt @ Wg[:W] + h @ Wg[W:] + bg)
        r, u = g[:, :H], g[:, H:]
        c = torch.tanh(xt @ Wc[:W] + (r * h) @ Wc[W:] + bc)
        live = (lens > t).to(x.dtype)[:, None]
        h = live * (u * h + (1 - u) * c) + (1 - live) * h
    return h


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def forward(P, batch, table, nbox_table, answer_masks, masks, model_type="vlmap_answer", rounding=True, witness=None):
    assert model_type in MODEL_TYPES, model_type
    sc = O.scope_names(model_type)
    wit = (lambda k: witness[k]) if witness is not None else (lambda k: None)
    idx = torch.from_numpy(np.asarray(batch["image_idx"])).long()
    q = torch.from_numpy(np.asarray(batch["q_intseq"])).long()
    lens = torch.from_numpy(np.asarray(batch["q_intseq_len"])).long()
    tgt = _t(batch["answer_target"])
    V = _t(table)[idx]
    nb = torch.from_numpy(np.asarray(nbox_table)).long()[idx]
    v = _fc_ln_relu(V, P, sc["v_linear_v"], rounding, wit("v_linear_v"))
    e = P[sc["embed"]][q]
    h = _gru(e, lens, P[sc["gru_gates"] + "/kernel"], P[sc["gru_gates"] + "/bias"], P[sc["gru_cand"] + "/kernel"],
             P[sc["gru_cand"] + "/bias"])
    qv = _fc_ln_relu(h, P, sc["q_linear_v"], rounding, wit("q_linear_v"))
    feat = v * qv[:, None, :] * _t(masks["att"]) / O.KEEP_ATT
    s = (feat * P[sc["score"] + "/fc/weights"][:, 0]).sum(-1) + P[sc["score"] + "/fc/biases"]     # H -> 1: a row kernel
    R = V.shape[1]
    s = s.masked_fill(torch.arange(R)[None, :] >= nb[:, None], float("-inf"))
    att = torch.softmax(s, dim=-1)
    p = (att[:, :, None] * V).sum(1)
    pl = _fc_ln_relu(p, P, sc["pooled_linear_l"], rounding, wit("pooled_linear_l"))
    ll = _fc_ln_relu(h, P, sc["q_linear_l"], rounding, wit("q_linear_l"))
    j = _fc_ln_relu(pl * ll, P, sc["joint_fc"], rounding, wit("joint_fc")) * _t(masks["joint"]) / O.KEEP_JOINT
    z = _fc(j, P, sc["head"], rounding, wit("head"))
    ell = torch.clamp(z, min=0) - z * tgt + torch.log1p(torch.exp(-z.abs()))
    if model_type in O.TRAIN_MASKED_LOSS:
        ell = ell * _t(answer_masks["train"])
    loss = ell.sum(-1).mean()
    mid = {"v_linear_v": v, "condition": h, "q_linear_v": qv, "att_score": att, "pooled_V_ft": p, "pooled_linear_l": pl,
           "l_linear_l": ll, "joint": j, "logit": z, "embed": e}
    return loss, mid


def loss_and_grads(params, batch, table, nbox_table, answer_masks, masks, model_type="vlmap_answer", rounding=True,
                   witness=None):
    """(loss, mid as numpy, grads as numpy, dx [B,T,W] of the un-aggregated embedding slices, the 13 report scalars).
    witness: {layer of ROUTED: {"x": the step's left operand, "d": its d_pre}} (arrays) -- see _Routed; every entry
    gains "log" = {"x": ..., "d": ...}, the normalised distance of the witnessed value from this reference's own."""
    if witness is not None:
        witness = {k: {"x": _t(np.asarray(w["x"])), "d": _t(np.asarray(w["d"])), "log": w.setdefault("log", {})}
                   for k, w in witness.items()}
        assert set(witness) == set(ROUTED)
    P = {k: _t(v).clone().requires_grad_(True) for k, v in params.items()}
    loss, mid = forward(P, batch, table, nbox_table, answer_masks, masks, model_type, rounding, witness)
    mid["embed"].retain_grad()
    loss.backward()
    tape = P.pop("_tape")
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    dx = mid["embed"].grad.numpy()
    midn = {k: v.detach().numpy() for k, v in mid.items()}
    sc = O.scope_names(model_type)
    midn["routed"] = {k: {"x": tape[sc[k]][0].detach().numpy(), "d": tape[sc[k]][1].grad.numpy()} for k in ROUTED}
    am64 = {k: np.asarray(v, dtype=np.float64) for k, v in answer_masks.items()}
    _, report, out, _ = O.loss_and_report(midn["logit"], np.asarray(batch["answer_target"], dtype=np.float64), am64, model_type)
    midn["pred"] = out["pred"]
    return float(loss.detach()), midn, grads, dx, report
