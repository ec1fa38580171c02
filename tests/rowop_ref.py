"""Float64 references of the row, index and optimiser kernels of include/vqa_hot.h that only the whole-model tests used
to reach (bi-directional encoder helpers, legacy-LSTM kernels, ablation kernels, LayerNorm + tanh, element-wise ops,
the embedding gradient, the report and the optimiser), and the comparators the op-level tests judge them with.

Each function states the header's contract in plain torch, in `dtype` (float64 by default; the comparator's own tests
also evaluate it in float32).  Backward passes are torch autograd of the forward, never a hand-derived formula.  Index
kernels are plain gathers / scatters over the clamped length min(max(len, 0), T).

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import torch

# The bounds of the GPU op tests.  They started at 2e-6 absolute on bounded transcendental outputs and 1e-5 of a row's
# max-abs on reductions and backward passes, and are tightened here to about 3x the worst error measured on an MI355X
# (tests/test_gpu_rowops_f64.py lists the measurements).  The float32 evaluations of tests/test_rowop_reference.py pass
# the same bounds, so they are not tighter than a correct float32 implementation allows.
ABS_BOUNDED = 5e-7     # gates, tanh outputs, h: elementwise absolute bound
PROB_RTOL = 4e-6       # softmax probabilities and their marginal: elementwise, relative to the value itself
ROW_RTOL = 1e-5        # the starting point; kept where the measured worst is above a third of it (the score sums)
RTOL = {               # per output: bound on max |err| over a row relative to the row's scale (check_rows)
    "score_fwd": 1e-5, "score_bwd d_pq": 1e-5, "score_bwd part_dw": 1e-5, "score_bwd d_al": 5e-6,
    "clip_adam m": 5e-6, "clip_adam v": 2e-6, "clip_adam p": 1e-6,
    "marginal_entropy dz": 3e-6, "marginal_entropy ent_row": 1e-6,
    "embed_bwd_len_det": 2e-6, "embed_bwd_len_det (atomics)": 2e-6, "embed2_bwd dlearn": 1e-6, "embed2_bwd slice_sq": 1e-6,
    "lstm_step_fwd c_new": 2e-6, "lstm_step_bwd dgates": 1e-6, "lstm_step_bwd dc_prev": 1e-6,
    "gru_step_bwd dr_pre": 1e-6, "gru_step_bwd du_pre": 1e-6, "gru_step_bwd dc_pre": 1e-6, "gru_step_bwd dh_acc": 1e-6,
    "reparam_fwd x": 1e-6, "reparam_fwd kl_row": 1e-6, "reparam_bwd dmean": 1e-6, "reparam_bwd dlog_sigma_sq": 1e-6,
    "tile_mul_bwd": 1e-6, "tile_mul_bwd accumulate": 1e-6, "tanh_bwd": 1e-6, "sumsq": 1e-6, "report_reduce": 1e-6,
    "extra_report report[13:16]": 1e-6,
}
for _a in ("relu", "tanh"):
    for _o in ("_fwd mean", "_fwd rstd", "_bwd dpre", "_bwd part_dgamma", "_bwd part_dbeta", "_bwd part_dbias"):
        RTOL["ln_act(%s)%s" % (_a, _o)] = 1e-6
RTOL["ln_act(relu)_fwd y"] = 1e-6     # the tanh form's y is bounded: ABS_BOUNDED
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8
ENT_EPS = 1e-8
LN_EPS = 1e-12
STAT_COUNT = 16
REPORT_COUNT = 13
# vqa_hot.h VQA_STAT_* order
(S_LOSS_TRAIN, S_LOSS_REPORT, S_ALL, S_EXIST, S_TEST, S_TEST_OBJ, S_TEST_ATTR, S_TRAIN_EXIST, S_MAX_EXIST,
 S_MAX_TRAIN_EXIST, S_TEST_OBJ_MAX, S_TEST_ATTR_MAX, S_TEST_MAX, S_TEST_MAX_EXIST, S_MAX_TRAIN) = range(15)


def f64(*ts, dtype=torch.float64):
    return [t.to(dtype) if t is not None else None for t in ts]


def clamp_len(lens, T):
    return lens.to(torch.long).clamp(0, T)


# ------------------------------------------------------------------------------------------------ bi-directional encoder
def reverse_tokens(q, lens):
    """q_rev[b, t] = q[b, n_b - 1 - t] for t < n_b, q[b, t] otherwise (n_b = clamped len)"""
    B, T = q.shape
    n = clamp_len(lens, T).to(q.device)[:, None]
    t = torch.arange(T, device=q.device)[None, :]
    src = torch.where(t < n, n - 1 - t, t)
    return torch.gather(q, 1, src)


def bi_outputs_fwd(hs_fw, hs_bw, lens):
    """hs_* [T+1,B,h] -> q_map [B,T,2h] (fw: hs_fw[t+1], bw: hs_bw[n-t], zero for t >= n), q_ft [B,2h]"""
    T1, B, h = hs_fw.shape
    T = T1 - 1
    n = clamp_len(lens, T).to(hs_fw.device)
    q_map = hs_fw.new_zeros(B, T, 2 * h)
    for b in range(B):
        for t in range(int(n[b])):
            q_map[b, t, :h] = hs_fw[t + 1, b]
            q_map[b, t, h:] = hs_bw[int(n[b]) - t, b]
    q_ft = torch.cat([hs_fw[T], hs_bw[T]], dim=1)
    return q_map, q_ft


def bi_outputs_bwd(d_map, d_ft, lens):
    """d_map [B,T,2h], d_ft [B,2h] -> dout_fw, dout_bw [T,B,h] (step order of each recurrence, zero for s >= n),
    dhT_fw, dhT_bw [B,h]"""
    B, T, h2 = d_map.shape
    h = h2 // 2
    n = clamp_len(lens, T).to(d_map.device)
    dout_fw, dout_bw = d_map.new_zeros(T, B, h), d_map.new_zeros(T, B, h)
    for b in range(B):
        nb = int(n[b])
        for s in range(nb):
            dout_fw[s, b] = d_map[b, s, :h]
            dout_bw[s, b] = d_map[b, nb - 1 - s, h:]
    return dout_fw, dout_bw, d_ft[:, :h].clone(), d_ft[:, h:].clone()


def bi_dx_combine(dx_fw, dx_bw, lens, dtype=torch.float64):
    """dx[t, b] = dx_fw[t, b] + dx_bw[n_b - 1 - t, b] (t < n_b), dx_fw[t, b] + dx_bw[t, b] otherwise"""
    T, B, W = dx_fw.shape
    n = clamp_len(lens, T).to(dx_fw.device)[None, :]
    t = torch.arange(T, device=dx_fw.device)[:, None]
    src = torch.where(t < n, n - 1 - t, t)                                   # [T,B]
    g = torch.gather(dx_bw, 0, src[:, :, None].expand(T, B, W))
    a, b = f64(dx_fw, g, dtype=dtype)
    return a + b


# ------------------------------------------------------------------------------------------------------------ ablations
def reparam_fwd(mean, ls, noise, dtype=torch.float64):
    """x = mean + noise sqrt(exp(ls)); kl_row = -0.5 sum_h (1 + ls - mean^2 - exp(ls)); also the natural scale of
    each kl_row sum (sum_h of the terms' magnitudes)"""
    m, l, z = f64(mean, ls, noise, dtype=dtype)
    e = torch.exp(l)
    x = m + z * torch.sqrt(e)
    terms = 1 + l - m * m - e
    return x, -0.5 * terms.sum(1), 0.5 * (1 + l.abs() + m * m + e).sum(1)


def reparam_bwd(dx, mean, ls, noise, coef, dtype=torch.float64):
    """autograd of <dx, x> + coef sum_b kl_row[b]  ->  (dmean, dls)"""
    with torch.enable_grad():
        m, l = (t.detach().to(dtype).requires_grad_(True) for t in (mean, ls))
        x, kl, _ = reparam_fwd(m, l, noise, dtype)
        loss = (dx.to(dtype) * x).sum() + coef * kl.sum()
        return torch.autograd.grad(loss, (m, l))


def outer_rows(att, dp, dtype=torch.float64):
    """out[b, r, :] = att[b, r] dp[b, :]"""
    a, d = f64(att, dp, dtype=dtype)
    return a[:, :, None] * d[:, None, :]


def tile_src(B, M, device=None):
    """source row of pl for output row (b, m): (b M + m) % B"""
    return torch.arange(B * M, device=device) % B


def tile_mul_fwd(pl, ll, M, dtype=torch.float64, src=None):
    """x[(b, m), :] = pl[(b M + m) % B, :] ll[b, :]  (src overrides the source rows: the comparator's tests)"""
    B = ll.shape[0]
    p, l = f64(pl, ll, dtype=dtype)
    s = tile_src(B, M, pl.device) if src is None else src
    return p[s] * l.repeat_interleave(M, dim=0)


def tile_mul_bwd(dx, pl, ll, M, dtype=torch.float64):
    """autograd of <dx, tile_mul_fwd(pl, ll)> wrt ll (pl is behind tf.stop_gradient)"""
    with torch.enable_grad():
        l = ll.detach().to(dtype).requires_grad_(True)
        (g,) = torch.autograd.grad((dx.to(dtype) * tile_mul_fwd(pl, l, M, dtype)).sum(), l)
    return g


def entropy_select(train, exist, cols):
    return (train[:cols].to(torch.float64) * exist[:cols].to(torch.float64)) > 0.5


def marginal_entropy(tz, train, exist, coef, B, M, cols, dtype=torch.float64, tamper=None):
    """tz [B*M, >= cols] logits.  Softmax over the selected answers of every pairing (0 elsewhere; every probability 0
    when no answer is selected), marginal [B, cols] = mean over the M pairings, ent_row [B] = sum_a marginal
    log(marginal + 1e-8) over the selected answers, dz [B*M, cols] = autograd of coef sum_b ent_row.  Returns
    (prob, marginal, ent_row, dz, ent_scale) with ent_scale = sum_a |marginal log(marginal + 1e-8)|.
    tamper(prob, marginal) -> marginal: a wrong marginal (the comparator's tests)."""
    sel = entropy_select(train, exist, cols).to(tz.device)
    with torch.enable_grad():
        z = tz[:, :cols].detach().to(dtype).requires_grad_(True)
        zs = z.masked_fill(~sel, float("-inf"))
        if bool(sel.any()):
            prob = torch.softmax(zs, dim=1).masked_fill(~sel, 0.0)
        else:
            prob = z * 0.0
        marg = prob.view(B, M, cols).mean(1)
        if tamper is not None:
            marg = tamper(prob, marg)
        pl = (marg * torch.log(marg + ENT_EPS)).masked_fill(~sel, 0.0)
        ent = pl.sum(1)
        (dz,) = torch.autograd.grad(coef * ent.sum(), z)
    return prob.detach(), marg.detach(), ent.detach(), dz, pl.detach().abs().sum(1)


def extra_report(extra_row, report0, weight, dtype=torch.float64):
    """report[13] = mean_b extra_row, [14] = weight * that, [15] = report[0] + [14]"""
    (e,) = f64(extra_row, dtype=dtype)
    mean = e.mean()
    return torch.stack([mean, weight * mean, float(report0) + weight * mean])


# ---------------------------------------------------------------------------------------------------------- legacy LSTM
def embed2_fwd(fixed, learn, ids, Vq):
    """x_tm [T,N,W]: id = clamp(ids[n, t], 0, Vq-1); row fixed[id] for id < Vq-3, learn[id - (Vq-3)] otherwise"""
    table = torch.cat([fixed[:Vq - 3], learn[:3]], 0)
    return table[ids.to(torch.long).clamp(0, Vq - 1)].transpose(0, 1)


def embed2_bwd(dx_tm, ids, Vq, dtype=torch.float64):
    """(dlearn [3,W], slice_sq): scatter-add of the rows dx_tm[t, n] with clamped id >= Vq-3 into dlearn[id-(Vq-3)],
    and the sum of squares of those un-aggregated rows"""
    T, N, W = dx_tm.shape
    (dx,) = f64(dx_tm, dtype=dtype)
    idx = ids.to(torch.long).clamp(0, Vq - 1).t().reshape(-1).to(dx.device)      # time-major, like dx_tm's rows
    rows = dx.reshape(T * N, W)
    hit = idx >= Vq - 3
    dlearn = dx.new_zeros(3, W).index_add_(0, idx[hit] - (Vq - 3), rows[hit])
    return dlearn, (rows[hit] ** 2).sum()


def lstm_cell(g, c_prev, forget_bias=1.0):
    """BasicLSTMCell on pre-activations g [N,4L] (i, j, f, o): (activated gates, c_new, h_new)"""
    L = g.shape[1] // 4
    i, j = torch.sigmoid(g[:, :L]), torch.tanh(g[:, L:2 * L])
    f, o = torch.sigmoid(g[:, 2 * L:3 * L] + forget_bias), torch.sigmoid(g[:, 3 * L:])
    c = c_prev * f + i * j
    return torch.cat([i, j, f, o], 1), c, torch.tanh(c) * o


def lstm_step_fwd(gates, c_prev, h_prev, lens, t, dtype=torch.float64, cell=lstm_cell):
    """(activated gates [N,4L], c_new, h_new): rows with t >= len carry (c, h) through"""
    g, c, h = f64(gates, c_prev, h_prev, dtype=dtype)
    act, cn, hn = cell(g, c)
    live = (lens.to(torch.long).to(g.device) > t)[:, None]
    return act, torch.where(live, cn, c), torch.where(live, hn, h)


def lstm_step_bwd(dh, dc, gates, c_prev, h_prev, lens, t, dtype=torch.float64):
    """autograd of <dh, h_new> + <dc, c_new> wrt (pre-activations, c_prev, h_prev) = (dgates, dc_prev, dh_carry)"""
    with torch.enable_grad():
        g, c, h = (x.detach().to(dtype).requires_grad_(True) for x in (gates, c_prev, h_prev))
        _, cn, hn = lstm_step_fwd(g, c, h, lens, t, dtype)
        loss = (dh.to(dtype) * hn).sum() + (dc.to(dtype) * cn).sum()
        return torch.autograd.grad(loss, (g, c, h))


def score_fwd(al, pq, w, bias, dtype=torch.float64):
    """z[b, a] = sum_k w[k] tanh(al[a, k] + pq[b, k]) + bias[0]"""
    a, p, ww, bb = f64(al, pq, w, bias, dtype=dtype)
    ww = ww.reshape(-1, a.shape[1])[:, None, :]                       # [1 or B, 1, L]
    return (torch.tanh(a[None, :, :] + p[:, None, :]) * ww).sum(-1) + bb.reshape(-1)[0]


def score_bwd(dz, al, pq, w, bias, dtype=torch.float64):
    """autograd of <dz, z> wrt al, pq and a per-question copy of w: (d_al [A,L], d_pq [B,L], part_dw [B,L])"""
    B = pq.shape[0]
    with torch.enable_grad():
        a, p = (x.detach().to(dtype).requires_grad_(True) for x in (al, pq))
        wb = w.detach().to(dtype).reshape(1, -1).repeat(B, 1).requires_grad_(True)
        z = score_fwd(a, p, wb, bias, dtype)
        return torch.autograd.grad((dz.to(dtype) * z).sum(), (a, p, wb))


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def ln_act_fwd(pre, gamma, beta, keepmask, keep_prob, G, rows, act, dtype=torch.float64):
    """y [G*rows,N] = act(layer_norm over each group of `rows` rows (biased variance, eps 1e-12) * gamma + beta)
    [* keepmask / keep_prob]; act 0 = ReLU, 1 = tanh.  Returns (y, mean [G], rstd [G], ln)."""
    x, ga, be = f64(pre, gamma, beta, dtype=dtype)
    N = x.shape[1]
    xg = x.reshape(G, rows * N)
    mean = xg.mean(1)
    var = ((xg - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    ln = ((xg - mean[:, None]) * rstd[:, None]).reshape(G * rows, N) * ga + be
    y = torch.relu(ln) if act == 0 else torch.tanh(ln)
    if keepmask is not None:
        y = y * keepmask.to(dtype) / keep_prob
    return y, mean, rstd, ln


def ln_act_bwd(dy, pre, gamma, beta, keepmask, keep_prob, G, rows, act, dtype=torch.float64):
    """autograd of <dy, y> wrt pre and per-group copies of gamma, beta and a bias added to pre:
    (dpre [G*rows,N], part_dgamma, part_dbeta, part_dbias [G,N])"""
    N = pre.shape[1]
    with torch.enable_grad():
        x = pre.detach().to(dtype).requires_grad_(True)
        ga = gamma.detach().to(dtype).reshape(1, N).repeat(G, 1).requires_grad_(True)
        be = beta.detach().to(dtype).reshape(1, N).repeat(G, 1).requires_grad_(True)
        bi = torch.zeros(G, N, dtype=dtype, device=pre.device, requires_grad=True)
        rep = lambda v: v.repeat_interleave(rows, dim=0)
        xx = x + rep(bi)
        xg = xx.reshape(G, rows * N)
        mean = xg.mean(1, keepdim=True)
        var = ((xg - mean) ** 2).mean(1, keepdim=True)
        ln = ((xg - mean) / torch.sqrt(var + LN_EPS)).reshape(G * rows, N) * rep(ga) + rep(be)
        y = torch.relu(ln) if act == 0 else torch.tanh(ln)
        if keepmask is not None:
            y = y * keepmask.to(dtype) / keep_prob
        return torch.autograd.grad((dy.to(dtype) * y).sum(), (x, ga, be, bi))


# ------------------------------------------------------------------------------------------------------ GRU step pieces
def gru_step_fwd(gpre, cpre, h_prev, lens, t, dtype=torch.float64):
    """one GRUCell step from its pre-activations gpre [B,>=2H] (r | u) and cpre [B,>=H]: (r, u, rh, c, h_new) with
    rh = r h_prev and h_new = u h_prev + (1 - u) c for t < len, h_prev otherwise"""
    H = h_prev.shape[1]
    g, cp, h = f64(gpre, cpre, h_prev, dtype=dtype)
    r, u = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H])
    c = torch.tanh(cp[:, :H])
    live = (lens.to(torch.long).to(h.device) > t)[:, None]
    return r, u, r * h, c, torch.where(live, u * h + (1 - u) * c, h)


def gru_step_bwd(dh, drh, gpre, cpre, h_prev, lens, t, dtype=torch.float64):
    """autograd of <dh, h_new> + <drh, rh> wrt (r, u, c pre-activations, h_prev): (dr_pre, du_pre, dc_pre, dh_prev).
    dh_prev is the direct part vqa_gru_bwd_a starts and vqa_gru_bwd_b completes (the caller adds the GEMM terms)."""
    H = h_prev.shape[1]
    with torch.enable_grad():
        rp, up, cp, h = (x.detach().to(dtype).requires_grad_(True)
                         for x in (gpre[:, :H], gpre[:, H:2 * H], cpre[:, :H], h_prev))
        _, _, rh, _, hn = gru_step_fwd(torch.cat([rp, up], 1), cp, h, lens, t, dtype)
        loss = (dh.to(dtype) * hn).sum() + (drh.to(dtype) * rh).sum()
        return torch.autograd.grad(loss, (rp, up, cp, h))


def im2col(x, kh, kw, stride, pad_t, pad_l, Ho, Wo, Kpad, mean=None):
    """col [B*Ho*Wo, Kpad]: col[(b, oy, ox), (ky kw + kx) Ci + ci] = x[b, oy s - pad_t + ky, ox s - pad_l + kx, ci]
    - mean[ci] for in-bounds pixels, 0 outside the image and in the K padding"""
    B, Hi, Wi, Ci = x.shape
    xx = x.to(torch.float64) - (torch.tensor(mean, dtype=torch.float64, device=x.device) if mean is not None else 0.0)
    big = xx.new_zeros(B, pad_t + (Ho - 1) * stride + kh, pad_l + (Wo - 1) * stride + kw, Ci)
    hh, ww = min(Hi, big.shape[1] - pad_t), min(Wi, big.shape[2] - pad_l)
    big[:, pad_t:pad_t + hh, pad_l:pad_l + ww] = xx[:, :hh, :ww]
    taps = [big[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            for ky in range(kh) for kx in range(kw)]                        # each [B,Ho,Wo,Ci]
    col = torch.stack(taps, 3).reshape(B * Ho * Wo, kh * kw * Ci)
    return torch.cat([col, col.new_zeros(col.shape[0], Kpad - col.shape[1])], 1)


# ------------------------------------------------------------------------------------------------ element-wise, gather
def embed_bwd_len(dx_tm, q, lens, Vq, dtype=torch.float64):
    """dE [Vq,W] = sum over positions t < len_b of dx[t, b] scattered to row clamp(q[b, t], 0, Vq-1)"""
    T, B, W = dx_tm.shape
    (dx,) = f64(dx_tm, dtype=dtype)
    idx = q.to(torch.long).clamp(0, Vq - 1).t().reshape(-1).to(dx.device)
    live = (torch.arange(T, device=dx.device)[:, None] < lens.to(torch.long).to(dx.device)[None, :]).reshape(-1)
    return dx.new_zeros(Vq, W).index_add_(0, idx[live], dx.reshape(T * B, W)[live])


def mul_bwd(dz, a, b, dtype=torch.float64):
    """autograd of <dz, a * b>: (da, db)"""
    with torch.enable_grad():
        x, y = (t.detach().to(dtype).requires_grad_(True) for t in (a, b))
        return torch.autograd.grad((dz.to(dtype) * x * y).sum(), (x, y))


def tanh_bwd(dy, y, dtype=torch.float64):
    """dx = dy (1 - y^2) (y = tanh(x) given)"""
    d, yy = f64(dy, y, dtype=dtype)
    return d * (1 - yy * yy)


# --------------------------------------------------------------------------------------------------- report, optimiser
def report_reduce(stats, dtype=torch.float64):
    """report [13]: column means of stats [B,16] and the guarded ratios where(den == 0, den, num / den); also the
    natural scale of each entry (mean |column| for the means, |ratio| for the ratios)"""
    (s,) = f64(stats, dtype=dtype)
    mean = s.mean(0)
    scale = s.abs().mean(0)
    ratio = lambda n, d: (mean[d] if float(mean[d]) == 0.0 else mean[n] / mean[d])
    idx = [S_LOSS_TRAIN, S_LOSS_REPORT, S_ALL, S_EXIST, S_TEST]
    ratios = [(S_TEST, S_TEST_MAX), (S_TEST_OBJ, S_TEST_OBJ_MAX), (S_TEST_ATTR, S_TEST_ATTR_MAX),
              (S_EXIST, S_MAX_EXIST), (S_TRAIN_EXIST, S_MAX_TRAIN_EXIST)]
    tail = [S_MAX_EXIST, S_TEST_MAX, S_TEST_MAX_EXIST]
    rep = [mean[k] for k in idx] + [ratio(n, d) for n, d in ratios] + [mean[k] for k in tail]
    sc = [scale[k] for k in idx] + [torch.as_tensor(r).abs() for r in rep[5:10]] + [scale[k] for k in tail]
    return torch.stack([torch.as_tensor(r, dtype=dtype) for r in rep]), torch.stack([torch.as_tensor(x, dtype=dtype)
                                                                                      for x in sc])


def sumsq(g, extra=None):
    (x,) = f64(g)
    s = (x * x).sum()
    return s + float(extra) if extra is not None else s


def adam_lr(lr, t, b1=ADAM_B1, b2=ADAM_B2):
    """TF1 Adam's bias-corrected rate lr sqrt(1 - b2^t) / (1 - b1^t), in float64"""
    return lr * (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t)


def clip_adam(p, g, m, v, norm, clip, lr_t, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS, dtype=torch.float64, tail=None):
    """one step of clip_by_global_norm + Adam: g' = g clip / max(norm, clip); m = b1 m + (1-b1) g';
    v = b2 v + (1-b2) g'^2; p -= lr_t m / (sqrt(v) + eps).  Returns new (p, m, v); inputs are not modified.
    tail(i) -> scale: a different clip scale for element i (the comparator's tests)"""
    p, g, m, v = f64(p, g, m, v, dtype=dtype)
    scale = clip / max(float(norm), clip)
    gs = g * scale
    if tail is not None:
        i, s = tail
        gs[i] = g[i] * s
    m = b1 * m + (1 - b1) * gs
    v = b2 * v + (1 - b2) * gs * gs
    return p - lr_t * m / (torch.sqrt(v) + eps), m, v


# --------------------------------------------------------------------------------------------------------- comparators
class Worst:
    """worst measured error per kernel and output, as a fraction of its bound (0 for bit-exact outputs): what the
    GPU tests report"""
    def __init__(self):
        self.d = {}

    def add(self, name, ratio):
        self.d[name] = max(self.d.get(name, 0.0), ratio)
        return ratio

    def table(self):
        return "\n".join("  %-28s %s" % (k, "bit-exact" if r == 0 else "%.3f of the bound" % r)
                         for k, r in sorted(self.d.items()))


def check_written(got, what):
    bad = ~torch.isfinite(got)
    if bool(bad.any()):
        first = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError("%s: %d values not written / not finite, first at %s" % (what, int(bad.sum()), first))


def check_bits(got, ref, what):
    """got equals ref (rounded to got's dtype) bit for bit"""
    if tuple(got.shape) != tuple(ref.shape):
        raise AssertionError("%s: shape %s, want %s" % (what, tuple(got.shape), tuple(ref.shape)))
    r = ref.to(got.dtype).to(got.device)
    if got.dtype.is_floating_point:
        ok = got.view(torch.int32) == r.view(torch.int32) if got.dtype == torch.float32 else got == r
    else:
        ok = got == r
    if not bool(ok.all()):
        first = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError("%s: %d elements differ from the reference, first at %s (got %r, want %r)"
                             % (what, int((~ok).sum()), first, got[first].item(), r[first].item()))
    return 0.0


def check_rows(got, ref, what, rtol=ROW_RTOL, atol=0.0, scale=None):
    """Judge `got` against the float64 `ref` row by row (row = index of the leading axis): fully written and finite,
    and max |err| over the row <= atol + rtol * scale_row, scale_row = the row's own max |ref| (or `scale` [rows]
    given).  An error confined to one row, one column block or one element cannot hide under the tensor's scale.
    Returns the worst err_row / bound_row; raises AssertionError with the failing rows."""
    if tuple(got.shape) != tuple(ref.shape):
        raise AssertionError("%s: shape %s, want %s" % (what, tuple(got.shape), tuple(ref.shape)))
    check_written(got, what)
    g = got.to(torch.float64).reshape(got.shape[0] if got.dim() else 1, -1)
    r = ref.to(torch.float64).to(got.device).reshape(g.shape)
    if g.numel() == 0:
        return 0.0
    err = (g - r).abs().amax(1)
    sc = r.abs().amax(1) if scale is None else scale.to(torch.float64).to(got.device).reshape(-1)
    bound = atol + rtol * sc
    bad = err > bound
    if bool(bad.any()):
        rows = bad.nonzero()[:, 0][:8].tolist()
        raise AssertionError("%s: %d of %d rows out of bounds:\n%s" % (
            what, int(bad.sum()), g.shape[0],
            "\n".join("  row %d err %.3e bound %.3e" % (i, float(err[i]), float(bound[i])) for i in rows)))
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    return float(ratio.max())


def check_elementwise(got, ref, what, rtol=PROB_RTOL):
    """every element within rtol of its own reference value (exact where the reference is 0)"""
    r = ref.to(torch.float64).to(got.device).reshape(-1, 1)
    return check_rows(got.reshape(-1, 1), r, what, rtol=rtol, scale=r.abs().reshape(-1))


def max_err(got, ref):
    return float((got.to(torch.float64) - ref.to(torch.float64).to(got.device)).abs().max()) if got.numel() else 0.0
