"""Float64 references of the loss heads (csrc/loss_optim.hip: vqa_loss_fwd, vqa_loss2_fwd, vqa_rowmin_mask_fwd/bwd,
vqa_softmax_ce_fwd, vqa_softmax_ce_pair_fwd) and of the paired LayerNorm (csrc/layernorm.hip: vqa_ln_pair_mul_fwd/bwd),
the case matrix the CPU and the GPU tests share, a restatement of the dispatch conditions, and the judges that hold an
implementation to the references with the comparators of tests/rowop_ref.py.

Each function states the header's contract in plain torch, in `dtype` (float64 by default).

  discrete   pred, top-1 and top-k are decided on the float32 values the kernel compares -- the logits as given, the
             float32 sum z + z2 (sum_mode 1 and SUM heads: the header forms it in float32), z (1 - train) + z2 train
             (sum_mode 0) -- so they are exact: bit for bit.  The first index wins a tie; the rank of the label is the
             number of entries larger than it, or equal with a lower index.
  scores     statistics 2..14 are products of a target and 0/1 masks: exact, bit for bit; statistic 15 is 0.
  gradients  torch autograd of the forward loss, never a formula (vqa_rowmin_mask_bwd: autograd of torch.amin, which
             splits evenly over ties -- tests/test_loss_reference.py holds it to the definition and finite differences).
  floats     |got - ref64| <= RT[output] * scale, scale = the sum of the magnitudes that enter the output, not the
             magnitude of the result (a gradient (sigmoid(x) - t) / B near 0 is the difference of two numbers near 0.5):
               loss sums      sum_a max(x, 0) + |x| t + log1p(exp(-|x|)) over the terms of the sum (masked where the
                              sum is masked)
               sigmoid dz     element by element, (sigmoid(x) + t) mask inv_batch per term
               softmax ce     max(1, max_a |z|) valid
               softmax dz     element by element, (p max(1, |z_a - lse|) + onehot) valid inv_valid_sum
               rowmin share   element by element, |dz| exist + sum_a |dz| (1 - exist); where exist == 1 and
                              z != rowmin the gradient keeps its bits
             RT is measured, not chosen: 8x the worst error / scale of this reference evaluated in float32 over the case
             matrix below (measure_rt; tests/test_loss_reference.py holds the table to the live measurement).  The
             float32 evaluation rounds every operation once (exp, log and the soft-plus are taken in float64 and
             rounded; sums run as a pairwise tree of float32 additions), so it gives the same bits on every CPU.

  output        float32 worst  RT = 8x    at
  loss sums     1.070e-07      8.561e-07  loss-A63-form2-random
  sigmoid dz    1.628e-07      1.303e-06  loss-A3000-form2-random
  softmax ce    1.016e-07      8.129e-07  softmax-A3-k5-most
  softmax dz    1.196e-07      9.572e-07  softmax-A3-k5-most
  rowmin share  4.922e-08      3.937e-07  rowmin-A3-random

vqa_ln_pair_mul_* is built on rowop_ref.ln_act_fwd/bwd and judged with the bounds tests/test_gpu_rowops_f64.py measured
for vqa_ln_act_*: rowop_ref.RTOL["ln_act(relu)..."] for y, mean, rstd, dpre and the partials, and twice the y bound
against rowmax|y_a| * rowmax|y_b| for z (two factors, each inside the y bound of its own row maximum).

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests import rowop_ref as R

U = 2.0 ** -24
F32_TINY = 2.0 ** -126
MEASURED = {
    "loss sums": (1.070e-07, "loss-A63-form2-random"),
    "sigmoid dz": (1.628e-07, "loss-A3000-form2-random"),
    "softmax ce": (1.016e-07, "softmax-A3-k5-most"),
    "softmax dz": (1.196e-07, "softmax-A3-k5-most"),
    "rowmin share": (4.922e-08, "rowmin-A3-random"),
}
RT = {k: 8 * v[0] for k, v in MEASURED.items()}
MASKS = ("train", "obj", "attr", "exist")
PAIR_MAX = 8


# ------------------------------------------------------------------------------------- once-rounded float32 operations
def _via64(op, x):
    return op(x) if x.dtype == torch.float64 else op(x.double()).to(x.dtype)


def _exp(x):
    return _via64(torch.exp, x)


def _log(x):
    return _via64(torch.log, x)


def _softplus(x):
    """log(1 + exp(x)) = max(x, 0) + log1p(exp(-|x|)), with the derivative sigmoid(x) at 0 too"""
    return _via64(lambda v: -F.logsigmoid(-v), x)


def _sum(x):
    """sum over the last axis: torch.sum in float64, a pairwise tree of float32 additions otherwise"""
    if x.dtype == torch.float64:
        return x.sum(-1)
    n = x.shape[-1]
    p = 1 << max(n - 1, 0).bit_length()
    if p != n:
        x = torch.cat([x, x.new_zeros(*x.shape[:-1], p - n)], -1)
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def first_argmax(x, last=False):
    """index of the first (last: the mutant) maximum of each row"""
    A = x.shape[1]
    idx = torch.arange(A, device=x.device)[None, :]
    hit = x == x.amax(1, keepdim=True)
    if last:
        return torch.where(hit, idx, -1).amax(1).to(torch.int32)
    return torch.where(hit, idx, A).amin(1).to(torch.int32)


def rank_of_label(x, label, ge=False):
    """entries tf.nn.top_k orders before the label: larger, or equal with a lower index (ge: every equal entry)"""
    lab = label.to(torch.long)[:, None]
    idx = torch.arange(x.shape[1], device=x.device)[None, :]
    zl = x.gather(1, lab)
    tie = (x == zl) & ((idx != lab) if ge else (idx < lab))
    return ((x > zl) | tie).sum(1)


# --------------------------------------------------------------------------------------------- sigmoid loss, two heads
def sigmoid_loss(z, tgt, masks, form=0, use_train_mask=1, inv_batch=1.0, z2=None, dtype=torch.float64, tamper=()):
    """form 0: vqa_loss_fwd; form 1: vqa_loss2_fwd with sum_mode 0 (z = fixed, z2 = tuned head); form 2: sum_mode 1.
    Returns stats [B,16], pred i32 [B], dz, dz2 (the gradients of inv_batch * sum_b stats[b, LOSS_TRAIN]), z_sum f32,
    and the scales loss_scale [B,2], dz_scale, dz2_scale.
    tamper: 'last_tie', 'sum_term_unmasked' (form 2), 'pred_from_sum' (form 1) -- the comparators' tests."""
    train, obj, attr, exist = (masks[k] for k in MASKS)
    tr, t = train.to(dtype), tgt.to(dtype)
    z_sum = (z + z2) if form else None                                         # float32
    with torch.enable_grad():
        x = z.detach().to(dtype).requires_grad_(True)
        ell = _softplus(x) - x * t
        mag = torch.relu(x) + x.abs() * t + (_softplus(x) - torch.relu(x))
        if form == 0:
            l_all, l_train = _sum(ell), _sum(ell * tr)
            s_all, s_train = _sum(mag), _sum(mag * tr)
            if not use_train_mask:
                l_train, s_train = l_all, s_all
            x2 = None
        else:
            x2 = z2.detach().to(dtype).requires_grad_(True)
            # sum_mode 1: the tuned term is the CE of the float32 sum (the header's z_sum); its gradient goes to both
            y = x2 if form == 1 else x + x2 + (z_sum.to(dtype) - (x + x2)).detach()
            ell2 = _softplus(y) - y * t
            mag2 = torch.relu(y) + y.abs() * t + (_softplus(y) - torch.relu(y))
            tr2 = torch.ones_like(tr) if (form == 1 or "sum_term_unmasked" in tamper) else tr
            l_all, l_train = _sum(ell + ell2), _sum(ell * tr + ell2 * tr2)
            s_all, s_train = _sum(mag + mag2), _sum(mag * tr + mag2 * tr2)
        grads = torch.autograd.grad(inv_batch * l_train.sum(), (x,) if x2 is None else (x, x2), allow_unused=True)
    dz = grads[0] if grads[0] is not None else torch.zeros_like(x)
    dz2 = grads[1] if form else None
    sg = lambda v: torch.sigmoid(v.detach().double())
    td, trd = tgt.double(), train.double()
    if form == 0:
        dz_scale = (sg(x) + td) * (trd if use_train_mask else 1.0) * inv_batch
        dz2_scale = None
        cmp32 = z
    elif form == 1:
        dz_scale, dz2_scale = (sg(x) + td) * trd * inv_batch, (sg(x2) + td) * inv_batch
        cmp32 = z_sum if "pred_from_sum" in tamper else z * (1.0 - train) + z2 * train        # float32
    else:
        dz2_scale = (sg(y) + td) * trd * inv_batch
        dz_scale = (sg(x) + td) * trd * inv_batch + dz2_scale
        cmp32 = z_sum
    pred = first_argmax(cmp32, last="last_tie" in tamper)
    B, A = z.shape
    te = 1.0 - tr
    tp = t.gather(1, pred.to(torch.long)[:, None])[:, 0]
    at = lambda m: m.to(dtype)[pred.to(torch.long)]
    ex, ob, a_ = exist.to(dtype), obj.to(dtype), attr.to(dtype)
    stats = torch.zeros(B, R.STAT_COUNT, dtype=dtype)
    stats[:, R.S_LOSS_TRAIN], stats[:, R.S_LOSS_REPORT] = l_train.detach(), l_all.detach()
    stats[:, R.S_ALL], stats[:, R.S_EXIST], stats[:, R.S_TEST] = tp, tp * at(exist), tp * (1 - at(train))
    stats[:, R.S_TEST_OBJ] = tp * (1 - at(train)) * at(obj)
    stats[:, R.S_TEST_ATTR] = tp * (1 - at(train)) * at(attr)
    stats[:, R.S_TRAIN_EXIST] = tp * at(exist) * at(train)
    stats[:, R.S_MAX_EXIST], stats[:, R.S_MAX_TRAIN_EXIST] = (t * ex).amax(1), (t * ex * tr).amax(1)
    stats[:, R.S_TEST_OBJ_MAX], stats[:, R.S_TEST_ATTR_MAX] = (t * te * ob).amax(1), (t * te * a_).amax(1)
    stats[:, R.S_TEST_MAX], stats[:, R.S_TEST_MAX_EXIST] = (t * te).amax(1), (t * ex * te).amax(1)
    stats[:, R.S_MAX_TRAIN] = (t * tr).amax(1)
    return dict(stats=stats, pred=pred, dz=dz, dz2=dz2, z_sum=z_sum,
                loss_scale=torch.stack([s_train.detach().double(), s_all.detach().double()], 1),
                dz_scale=dz_scale, dz2_scale=dz2_scale)


def _elementwise(got, ref, what, rtol, scale):
    """every element against its own scale; F32_TINY absolute, for a value under float32's normal range, which may
    be flushed to 0 (sigmoid(-110) = 1.7e-48)"""
    return R.check_rows(got.reshape(-1, 1), ref.reshape(-1, 1), what, rtol=rtol, atol=F32_TINY, scale=scale.reshape(-1))


def judge_loss(got, ref, what, rt=None):
    """got: stats, pred and, when the call asked for them, dz, dz2, z_sum.  Returns {output: worst err / bound}."""
    rt = RT if rt is None else rt
    out = {}
    R.check_bits(got["pred"], ref["pred"], what + " pred")
    R.check_written(got["stats"], what + " stats")
    R.check_bits(got["stats"][:, 2:], ref["stats"][:, 2:], what + " stats[2:16]")
    out["loss sums"] = max(R.check_rows(got["stats"][:, k:k + 1], ref["stats"][:, k:k + 1], "%s stats[%d]" % (what, k),
                                        rtol=rt["loss sums"], scale=ref["loss_scale"][:, k]) for k in (0, 1))
    for k in ("dz", "dz2"):
        if got.get(k) is not None:
            out["sigmoid dz"] = max(out.get("sigmoid dz", 0.0), _elementwise(got[k], ref[k], what + " " + k,
                                                                             rt["sigmoid dz"], ref[k + "_scale"]))
    if got.get("z_sum") is not None:
        R.check_bits(got["z_sum"], ref["z_sum"], what + " z_sum")
    return out


# ------------------------------------------------------------------------------------------------- row-minimum masking
def rowmin_mask_fwd(z, exist, dtype=torch.float64):
    """z_masked = z exist + rowmin(z) (1 - exist), rowmin [B]"""
    x, e = z.to(dtype), exist.to(dtype)
    m = torch.amin(x, 1)
    return x * e + m[:, None] * (1 - e), m


def rowmin_mask_bwd(dz, z, exist, dtype=torch.float64, tamper=()):
    """autograd of <dz, z_masked> wrt z, and its element-wise scale.  <dz, z_masked> is written as
    sum dz z exist + rowmin sum_a dz (1 - exist), so that the one sum of the gradient runs in this file's order.
    tamper 'whole_to_every_tie': the minimum's gradient is not split (the comparators' tests)."""
    d, e = dz.to(dtype), exist.to(dtype)
    with torch.enable_grad():
        x = z.detach().to(dtype).requires_grad_(True)
        m = torch.amin(x, 1)
        share = _sum(d * (1 - e))
        (g,) = torch.autograd.grad((d * e * x).sum() + (m * share).sum(), x)
    if "whole_to_every_tie" in tamper:
        g = d * e + (x.detach() == m.detach()[:, None]).to(dtype) * share[:, None]
    scale = dz.double().abs() * exist.double() + (dz.double().abs() * (1 - exist.double())).sum(1, keepdim=True)
    return g, scale


def judge_rowmin_bwd(got, ref, scale, dz_in, z, exist, what, rt=None):
    rt = RT if rt is None else rt
    keep = (exist[None, :] == 1) & (z != z.amin(1, keepdim=True))
    R.check_bits(got[keep], dz_in[keep], what + ": dz of existing answers away from the minimum")
    return {"rowmin share": _elementwise(got, ref, what, rt["rowmin share"], scale)}


# ----------------------------------------------------------------------------------------------------- softmax CE heads
def softmax_ce(z, label, valid, topk, inv_valid_sum, z2=None, dtype=torch.float64, tamper=()):
    """vqa_softmax_ce_fwd of z, or of the float32 sum z + z2 (a SUM head).  Returns stats [rows,4] =
    {ce valid, top1 valid, topk valid, valid}, dz = autograd of inv_valid_sum sum_r ce_r valid_r, and the scales.
    tamper: 'last_tie', 'rank_ge', 'no_inv_scale', 'invalid_rows_written', 'padding_lane'."""
    x32 = z if z2 is None else z + z2
    lab = label.to(torch.long)
    v = valid.to(dtype)
    inv = float(inv_valid_sum)
    with torch.enable_grad():
        x = x32.detach().to(dtype).requires_grad_(True)
        mx = x.detach().amax(1, keepdim=True)
        se = _sum(_exp(x - mx))
        if "padding_lane" in tamper:                       # a lane past the row's end counted as a logit of 0
            se = se + _exp(-mx[:, 0])
        lse = mx[:, 0] + _log(se)
        ce = lse - x.gather(1, lab[:, None])[:, 0]
        w = v * (1.0 if "no_inv_scale" in tamper else inv)
        if "invalid_rows_written" in tamper:
            w = torch.full_like(v, inv)
        (dz,) = torch.autograd.grad((ce * w).sum(), x)
    pred = first_argmax(x32, last="last_tie" in tamper).to(torch.long)
    rank = rank_of_label(x32, label, ge="rank_ge" in tamper)
    stats = torch.stack([ce.detach() * v, (pred == lab).to(dtype) * v, (rank < topk).to(dtype) * v, v], 1)
    xd, vd = x32.double(), valid.double()
    lse64 = torch.logsumexp(xd, 1, keepdim=True)
    onehot = F.one_hot(lab, x32.shape[1]).double()
    dz_scale = (torch.exp(xd - lse64) * (xd - lse64).abs().clamp(min=1.0) + onehot) * vd[:, None] * inv
    return dict(stats=stats, dz=dz, ce_scale=xd.abs().amax(1).clamp(min=1.0) * vd, dz_scale=dz_scale)


def judge_softmax(got, ref, what, rt=None):
    """got: stats and, when the call asked for it, dz"""
    rt = RT if rt is None else rt
    R.check_written(got["stats"], what + " stats")
    R.check_bits(got["stats"][:, 1:], ref["stats"][:, 1:], what + " stats[1:4] (top-1, top-k, valid)")
    out = {"softmax ce": R.check_rows(got["stats"][:, :1], ref["stats"][:, :1], what + " ce", rtol=rt["softmax ce"],
                                      scale=ref["ce_scale"])}
    if got.get("dz") is not None:
        out["softmax dz"] = _elementwise(got["dz"], ref["dz"], what + " dz", rt["softmax dz"], ref["dz_scale"])
    return out


# --------------------------------------------------------------------------------------------------------- paired LN
def ln_pair_mul_fwd(pre_a, pre_b, gamma_a, beta_a, gamma_b, beta_b, dtype=torch.float64):
    """LayerNorm + ReLU of both [G,N] pre-activations (one row per group) and z = y_a y_b"""
    G = pre_a.shape[0]
    ya, ma, ra, _ = R.ln_act_fwd(pre_a, gamma_a, beta_a, None, 1.0, G, 1, 0, dtype)
    yb, mb, rb, _ = R.ln_act_fwd(pre_b, gamma_b, beta_b, None, 1.0, G, 1, 0, dtype)
    return dict(y_a=ya, y_b=yb, z=ya * yb, mean_a=ma, rstd_a=ra, mean_b=mb, rstd_b=rb)


def ln_pair_mul_bwd(dz, add_b, pre_a, pre_b, gamma_a, beta_a, gamma_b, beta_b, dtype=torch.float64, tamper=()):
    """autograd of <dz, y_a y_b> + <add_b, y_b> wrt both pre-activations and the per-row copies of gamma, beta and a
    bias: dpre_*, part_dgamma_*, part_dbeta_*, part_dbias_* [G,N].  tamper 'add_b_on_a': the comparators' tests."""
    G = pre_a.shape[0]
    f = ln_pair_mul_fwd(pre_a, pre_b, gamma_a, beta_a, gamma_b, beta_b, dtype)
    with torch.enable_grad():
        ya, yb = (f[k].detach().requires_grad_(True) for k in ("y_a", "y_b"))
        loss = (dz.to(dtype) * ya * yb).sum()
        if add_b is not None:
            loss = loss + (add_b.to(dtype) * (ya if "add_b_on_a" in tamper else yb)).sum()
        dya, dyb = torch.autograd.grad(loss, (ya, yb))
    out = {}
    for s, dy, pre, ga, be in (("a", dya, pre_a, gamma_a, beta_a), ("b", dyb, pre_b, gamma_b, beta_b)):
        names = ("dpre_", "part_dgamma_", "part_dbeta_", "part_dbias_")
        out.update({n + s: v for n, v in zip(names, R.ln_act_bwd(dy, pre, ga, be, None, 1.0, G, 1, 0, dtype))})
    return out


def ln_inputs(G, N, rng):
    """pre-activations of growing scale per row, gamma around 1, small beta; every LayerNorm output within 1e-3 of the
    ReLU kink is moved 3e-3 away from it (where the float32 sign could differ from the float64 one): the method of
    tests/test_gpu_rowops_f64.py::_ln_inputs"""
    pre = torch.from_numpy(rng.standard_normal((G, N)).astype(np.float32)) * (1 + torch.arange(G)[:, None]) + 0.5
    gamma = torch.from_numpy((0.75 + 0.5 * rng.random(N)).astype(np.float32))
    beta = torch.from_numpy((0.2 * rng.standard_normal(N)).astype(np.float32))
    _, _, rstd, ln = R.ln_act_fwd(pre, gamma, beta, None, 1.0, G, 1, 0)
    shift = 3e-3 * torch.where(ln >= 0, 1.0, -1.0) / (gamma.double() * rstd[:, None])
    pre = (pre.double() + torch.where(ln.abs() < 1e-3, shift, torch.zeros_like(shift))).float()
    _, _, _, ln = R.ln_act_fwd(pre, gamma, beta, None, 1.0, G, 1, 0)
    assert float(ln.abs().min()) > 1e-5
    return pre, gamma, beta


LN_Y = "ln_act(relu)_fwd y"


def judge_ln_pair_fwd(got, ref, pre_a, pre_b, what):
    out = {}
    for s, pre in (("a", pre_a), ("b", pre_b)):
        out["ln_pair y_" + s] = R.check_rows(got["y_" + s], ref["y_" + s], what + " y_" + s, rtol=R.RTOL[LN_Y])
        out["ln_pair mean_" + s] = R.check_rows(got["mean_" + s], ref["mean_" + s], what + " mean_" + s,
                                                rtol=R.RTOL["ln_act(relu)_fwd mean"], scale=pre.abs().amax(1))
        out["ln_pair rstd_" + s] = R.check_rows(got["rstd_" + s], ref["rstd_" + s], what + " rstd_" + s,
                                                rtol=R.RTOL["ln_act(relu)_fwd rstd"])
    out["ln_pair z"] = R.check_rows(got["z"], ref["z"], what + " z", rtol=2 * R.RTOL[LN_Y],
                                    scale=ref["y_a"].abs().amax(1) * ref["y_b"].abs().amax(1))
    return out


def judge_ln_pair_bwd(got, ref, what):
    """got holds the outputs the call asked for; part_dbias is judged against the row's max |dpre| (one row per group)"""
    out = {}
    for k, g in got.items():
        if g is None:
            continue
        base = k[:-2]
        kw = dict(scale=ref["dpre_" + k[-1]].abs().amax(1)) if base == "part_dbias" else {}
        out["ln_pair " + k] = R.check_rows(g, ref[k], what + " " + k, rtol=R.RTOL["ln_act(relu)_bwd " + base], **kw)
    return out


# ------------------------------------------------------------------------------------------------------------ dispatch
def loss_kernel_form(entry, sum_mode=0):
    """template argument of loss_fwd_kernel: vqa_loss_fwd -> 0; vqa_loss2_fwd -> 1 (sum_mode 0), 2 (sum_mode != 0)"""
    return 0 if entry == "loss_fwd" else (2 if sum_mode else 1)


def softmax_route(A, fast=1, aligned=True):
    """'three-pass', or the NV of the register-resident row: A % 4 == 0, A <= 4096, every block 16-byte aligned and
    vqa_softmax_set_fast(1); NV = ceil(A / 4 / 256)"""
    if fast and A % 4 == 0 and A <= 4096 and aligned:
        return min((A // 4 + 255) // 256, 4)
    return "three-pass"


def ln_pair_vpt(N):
    """float4s per thread of vqa_ln_pair_mul_*: None where the entry point refuses (N % 4 != 0, N > 4096)"""
    if N <= 0 or N % 4 or N > 4096:
        return None
    return 1 if N <= 1024 else (2 if N <= 2048 else 4)


# --------------------------------------------------------------------------------------------------------- case matrix
LOSS_A = (1, 3, 63, 64, 65, 255, 256, 257, 513, 3000)
LOSS_B = 9
SOFTMAX_A = (1, 3, 4, 8, 37, 1020, 1024, 1028, 2048, 2052, 3072, 3076, 4096, 4100)
SOFTMAX_ROWS = 9
PAIR_A = (37, 40, 1028, 2052, 3076)          # three-pass (ragged), NV 1, 2, 3, 4
LN_N = (4, 16, 1020, 1024, 1028, 2048, 2052, 4092, 4096)
LN_G = (1, 5)


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def loss_cases():
    """(A, form, use_train_mask, mask kind): every A with random masks, all-0 and all-1 masks at A = 3 and 257"""
    out = []
    for A in LOSS_A:
        for form, utm in ((0, 1), (0, 0), (1, 1), (2, 1)):
            out.append((A, form, utm, "random"))
            if A in (3, 257):
                out += [(A, form, utm, "zeros"), (A, form, utm, "ones")]
    return out


def loss_id(A, form, utm, kind):
    return "loss-A%d-form%d%s-%s" % (A, form, "" if utm else "-unmasked", kind)


def _plant_tie(z, row, i, j, A, value):
    if j >= A:
        i, j = 0, A - 1
    z[row, i] = z[row, j] = value
    return (i, j)


def loss_inputs(A, form, kind, seed=0):
    """B = 9 rows.  0: all logits equal (pred 0); 1, 2, 3: tied maxima at (5, 5 + 256), (63, 64), (255, 256) -- at
    (0, A - 1) where A is too small; 4: the maximum at A - 1; 5: two heads: a tie that exists only in the logit the
    prediction is taken from (random masks, A >= 3); 6: |z| up to 60, both signs; 7: sparse targets; 8: fractional
    targets everywhere.  Returns z, z2 (None for form 0), tgt, masks, and the planted ties [(row, first, second)]."""
    rng = np.random.default_rng(1000 * A + 10 * form + seed)
    B = LOSS_B
    z = 3.0 * rng.standard_normal((B, A))
    z2 = 3.0 * rng.standard_normal((B, A)) if form else None
    if kind == "random":
        masks = {k: (rng.random(A) < 0.5).astype(np.float32) for k in MASKS}
    else:
        masks = {k: np.full(A, 0.0 if kind == "zeros" else 1.0, np.float32) for k in MASKS}
    ti, tj = A // 3, (2 * A) // 3
    if kind == "random" and A >= 3:
        masks["train"][ti], masks["train"][tj] = 0.0, 1.0
    z[0] = 0.25
    ties = []
    if form == 0:
        for row, (i, j) in ((1, (5, 261)), (2, (63, 64)), (3, (255, 256))):
            ties.append((row,) + _plant_tie(z, row, i, j, A, 20.0))
    else:
        z2[0] = 0.25
        # the tie must hold in the compared logit: both heads carry it (exact sums; either head under the train mask)
        for row, (i, j) in ((1, (5, 261)), (2, (63, 64)), (3, (255, 256))):
            ii, jj = _plant_tie(z, row, i, j, A, 20.0)
            z2[row, ii] = z2[row, jj] = 20.0
            ties.append((row, ii, jj))
        if kind == "random" and A >= 3:
            if form == 2:       # 30 + 10 == 10 + 30: neither head has the tie
                z[5, ti], z2[5, ti], z[5, tj], z2[5, tj] = 30.0, 10.0, 10.0, 30.0
            else:               # train[ti] = 0 takes the fixed head, train[tj] = 1 the tuned one
                z[5, ti], z2[5, ti], z[5, tj], z2[5, tj] = 40.0, -7.0, -9.0, 40.0
            ties.append((5, ti, tj))
    z[4, A - 1] = 25.0
    if form:
        z2[4, A - 1] = 25.0
    z[6] = rng.uniform(-60.0, 60.0, A)
    if A >= 2:
        z[6, 0], z[6, A - 1] = 60.0, -60.0
    if form:
        z2[6] = rng.uniform(-60.0, 60.0, A)
    tgt = rng.random((B, A)) * (rng.random((B, A)) < 0.4)
    tgt[8] = rng.random(A)
    tgt[7] = (rng.random(A) < 0.02) * 1.0
    return dict(z=_t(z), z2=_t(z2) if form else None, tgt=_t(tgt), masks={k: _t(v) for k, v in masks.items()}, ties=ties)


def rowmin_cases():
    out = []
    for A in LOSS_A:
        out.append((A, "random"))
        if A in (3, 257, 3000):
            out += [(A, "zeros"), (A, "ones")]
    return out


def rowmin_id(A, kind):
    return "rowmin-A%d-%s" % (A, kind)


def rowmin_inputs(A, kind):
    """B = 9 rows.  0: the minimum at an existing answer; 1: at a non-existing one; 2: a two-way tie (0, A - 1);
    3: a three-way tie (5, 5 + 256, A - 1), or (0, A // 2, A - 1); 4: an A-way tie; 5: a tie in neighbouring lanes of
    two waves (63, 64); 6..8: random.  exist[A // 3] = 1 and exist[2 A // 3] = 0 under random masks."""
    rng = np.random.default_rng(77 + A)
    B = LOSS_B
    z = 3.0 * rng.standard_normal((B, A))
    exist = (rng.random(A) < 0.5).astype(np.float32) if kind == "random" else np.full(A, float(kind == "ones"), np.float32)
    e1, e0 = A // 3, (2 * A) // 3
    if kind == "random" and A >= 3:
        exist[e1], exist[e0] = 1.0, 0.0
    z[0, e1] = -30.0
    z[1, e0] = -30.0
    z[2, [0, A - 1]] = -30.0
    z[3, [5, 261, A - 1] if A > 262 else [0, A // 2, A - 1]] = -30.0
    z[4] = -1.5
    if A > 64:
        z[5, [63, 64]] = -30.0
    dz = rng.standard_normal((B, A))
    return dict(z=_t(z), exist=_t(exist), dz=_t(dz))


def softmax_cases():
    return [(A, topk, v) for A in SOFTMAX_A for topk, v in ((5, "most"), (1, "most"), (5, "single"))]


def softmax_variants(A):
    """(fast, floats z is offset by, floats dz is offset by) of the calls the GPU test makes at one A: both settings of
    vqa_softmax_set_fast, and for A % 4 == 0 a z and, separately, a dz that is not 16-byte aligned"""
    return [(1, 0, 0), (0, 0, 0)] + ([(1, 1, 0), (1, 0, 1)] if A % 4 == 0 else [])


def softmax_id(A, topk, vkind):
    return "softmax-A%d-k%d-%s" % (A, topk, vkind)


def softmax_inputs(A, topk, vkind, seed=0):
    """9 rows.  0: label 0; 1: label A - 1 in a row shifted by +1000; 2: the label is the second of two tied maxima;
    3 / 4: the label's rank is exactly topk - 1 / topk, no ties; 5 / 6: the same with entries equal to the label on
    both sides of it (the lower ones are ranked before it, the higher ones are not); 7: valid 0 ('most'); 8: spread 80.
    Rows 3..6 are planted for A >= topk + 3, else left random (topk > A for the smallest A).  vkind 'single': row 3 is
    the only valid one, inv_valid_sum = 1."""
    rng = np.random.default_rng(31 * A + topk + seed)
    rows = SOFTMAX_ROWS
    z = 2.0 * rng.standard_normal((rows, A))
    label = rng.integers(0, A, rows)
    label[0], label[1] = 0, A - 1
    z[1] += 1000.0
    if A >= 2:
        i, j = sorted(rng.choice(A, 2, replace=False))
        z[2, i] = z[2, j] = 9.0
        label[2] = j
    if A >= topk + 3:
        L = A - 2
        for row, counted, tied in ((3, topk - 1, 0), (4, topk, 0), (5, topk - 1, max(topk - 2, 0)), (6, topk, 1)):
            v = 1.0
            z[row] = v - 0.5 - np.abs(z[row])
            z[row, L] = v
            label[row] = L
            lower = np.unique(np.linspace(0, L - 1, counted).round().astype(int)) if counted else np.array([], int)
            assert len(lower) == counted
            z[row, lower] = v + 1.0 + rng.random(counted)
            z[row, lower[:tied]] = v                       # equal, lower index: ranked before the label
            if row >= 5:
                z[row, A - 1] = v                          # equal, higher index: not ranked before it
    z[8] = rng.permutation(np.linspace(-40.0, 40.0, A)) if A > 1 else 40.0
    valid = np.ones(rows, np.float32)
    if vkind == "most":
        valid[7] = 0.0
    else:
        valid[:] = 0.0
        valid[3] = 1.0
    return dict(z=_t(z), label=_t(label, np.int32), valid=_t(valid), inv=1.0 / float(valid.sum()))      # 1/8 or 1: exact


# pair launches: name -> (A, [(split, misaligned block or None)]), one entry per head
def pair_cases():
    out = {}
    for A in PAIR_A:
        out["pair-A%d-mixed" % A] = (A, [(0, None), (1, None), (0, None)])
    out["pair-A1028-8split"] = (1028, [(1, None)] * PAIR_MAX)
    out["pair-A2052-misaligned"] = (2052, [(1, None), (0, "dzl"), (1, None)])
    return out


def pair_inputs(A, heads, seed=0):
    """3 rows per block: row 1 is invalid in every other head"""
    rng = np.random.default_rng(5 * A + len(heads) + seed)
    rows = 3
    out = []
    for h, (split, _) in enumerate(heads):
        valid = np.ones(rows, np.float32)
        if h % 2:
            valid[1] = 0.0
        out.append(dict(zv=_t(2.0 * rng.standard_normal((rows, A))), zl=_t(2.0 * rng.standard_normal((rows, A))),
                        label=_t(rng.integers(0, A, rows), np.int32), valid=_t(valid),
                        inv=float(np.float32(1.0 / valid.sum())),      # the float32 scalar the kernel reads
                        split=split))
    return out


def pair_tasks(head, topk, dtype=torch.float64, tamper=()):
    """the CEs of one head: [(stats name, dz names, reference)]"""
    if head["split"]:
        return [("stats_v", ("dzv",), softmax_ce(head["zv"], head["label"], head["valid"], topk, head["inv"], None, dtype, tamper)),
                ("stats_l", ("dzl",), softmax_ce(head["zl"], head["label"], head["valid"], topk, head["inv"], None, dtype, tamper))]
    return [("stats_v", ("dzv", "dzl"), softmax_ce(head["zv"], head["label"], head["valid"], topk, head["inv"], head["zl"],
                                                   dtype, tamper))]


def judge_pair_head(got, head, topk, what, want_dz=True, rt=None):
    """got: stats_v, stats_l, dzv, dzl of one head (float32).  A SUM head leaves stats_l alone; without gradients dzv
    and dzl are left alone: both must keep their NaN poison."""
    out = {}
    for sname, dnames, ref in pair_tasks(head, topk):
        for d in dnames if want_dz else (None,):
            g = dict(stats=got[sname], dz=got[d] if d else None)
            for k, r in judge_softmax(g, ref, "%s %s %s" % (what, sname, d or ""), rt).items():
                out[k] = max(out.get(k, 0.0), r)
    if not head["split"]:
        assert bool(torch.isnan(got["stats_l"]).all()), what + ": a SUM head wrote stats_l"
    if not want_dz:
        assert bool(torch.isnan(got["dzv"]).all()) and bool(torch.isnan(got["dzl"]).all()), what + ": dz written"
    return out


# ------------------------------------------------------------------------------------------ float32 evaluations (RT)
def f32_loss(A, form, utm, kind):
    d = loss_inputs(A, form, kind)
    kw = dict(form=form, use_train_mask=utm, inv_batch=1.0 / LOSS_B, z2=d["z2"])
    ref = sigmoid_loss(d["z"], d["tgt"], d["masks"], **kw)
    got = sigmoid_loss(d["z"], d["tgt"], d["masks"], dtype=torch.float32, **kw)
    return got, ref


def f32_rowmin(A, kind):
    d = rowmin_inputs(A, kind)
    ref, scale = rowmin_mask_bwd(d["dz"], d["z"], d["exist"])
    got, _ = rowmin_mask_bwd(d["dz"], d["z"], d["exist"], dtype=torch.float32)
    return got, ref, scale, d


def f32_softmax(A, topk, vkind):
    d = softmax_inputs(A, topk, vkind)
    ref = softmax_ce(d["z"], d["label"], d["valid"], topk, d["inv"])
    got = softmax_ce(d["z"], d["label"], d["valid"], topk, d["inv"], dtype=torch.float32)
    return got, ref


def measure_rt(rt=None):
    """worst err / scale of the float32 evaluation of every reference over the case matrix: {output: (worst, case)}.
    rt None: only measure (every bound at 1 x scale); else also raise where an evaluation leaves rt x scale."""
    unit = {k: 1.0 for k in MEASURED}
    worst = {k: (0.0, "") for k in MEASURED}

    def note(res, case):
        for k, r in res.items():
            if r > worst[k][0]:
                worst[k] = (r, case)

    def run(judge, case):
        if rt is not None:
            judge(rt)
        return judge(unit)

    for c in loss_cases():
        got, ref = f32_loss(*c)
        note(run(lambda b: judge_loss(got, ref, loss_id(*c), b), loss_id(*c)), loss_id(*c))
    for c in rowmin_cases():
        got, ref, scale, d = f32_rowmin(*c)
        note(run(lambda b: judge_rowmin_bwd(got, ref, scale, d["dz"], d["z"], d["exist"], rowmin_id(*c), b), rowmin_id(*c)),
             rowmin_id(*c))
    for c in softmax_cases():
        got, ref = f32_softmax(*c)
        note(run(lambda b: judge_softmax(got, ref, softmax_id(*c), b), softmax_id(*c)), softmax_id(*c))
    return worst
