"""Float64 reference of the bf16 mixed-precision mode of the cfg-5 pre-training step (include/vqa_hot.h,
VQA_FLAG_BF16_GEMM; PretrainEngine(precision="bf16")).

TEST INFRASTRUCTURE ONLY.  A torch restatement of oracle/pretrain_oracle.py's model (both LayerNorm modes) in the shape
the step computes it: the four heads' rows stacked (head h = 2 r + k, type rank r of (bf, ws), category k), every shared
layer ONE product over the stack -- pooled_linear_l over the 2 B n pooled rows, whose pre-activation both heads of a
category read, so that their d_pre meet BEFORE the one dW / dx, as in the step.  The routed products (forward, dW, dx of
pooled_linear_l, q_linear_l, joint_fc and the classifier) go through tests/bf16_ref.py's _Routed, which rounds both
operands of each of its three products; everything else -- the spatial attention (K = 6), wordset_ft (K = W), the caption
encoder, LayerNorm, the loss -- is plain float64.  With `rounding=False` it is oracle.pretrain_oracle.torch_loss_and_grads
(tests/test_pretrain_bf16_ref.py holds it to that).  `rounding=` and `witness=` as bf16_ref.loss_and_grads.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pretrain_oracle as PO
from oracle import vqa_oracle as O
from tests.bf16_ref import _Routed

# the routed layers in the order of the header's list; witness / mid["routed"] keys
ROUTED = ("pooled_linear_l", "q_linear_l", "joint_fc", "classifier")
HEADS = ("bf", "ws")

# (B, n, R, D, H, W, A, L) of the cases of tests/test_gpu_pretrain_bf16.py, and the vocabularies
CASES = {"toy": (3, 2, 5, 24, 16, 12, 21, 4),
         "medium": (8, 5, 36, 256, 128, 300, 300, 10),
         "full_dims": (4, 5, 36, 2048, 1024, 300, 4000, 10)}
VOCAB = {"toy": (20, 7), "medium": (200, 50), "full_dims": (500, 100)}        # (Vq, n_ws)
CASE_SEED = 21


def make_case(name, ln_shared=True, seed=CASE_SEED):
    """(params, batch, masks, dims) of a named case: float32 arrays from the oracle's generators"""
    B, n, R, D, H, W, A, L = CASES[name]
    Vq, n_ws = VOCAB[name]
    rng = np.random.default_rng(seed)
    p = PO.init_params(rng, Vq, n_ws, A, W=W, D=D, H=H, ln_shared=ln_shared)
    batch = PO.make_batch(rng, B, n, R, D, L, Vq, n_ws, A)
    masks = PO.make_masks(rng, B, n, R, H)
    return p, batch, masks, dict(B=B, n=n, R=R, D=D, H=H, W=W, A=A, L=L, Vq=Vq, n_ws=n_ws)


def to64(d):
    return {k: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in d.items()}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(torch.float64)


def _gru(x, lens, P):
    Wg, bg = P["encode_L_blank/rnn/gru_cell/gates/kernel"], P["encode_L_blank/rnn/gru_cell/gates/bias"]
    Wc, bc = P["encode_L_blank/rnn/gru_cell/candidate/kernel"], P["encode_L_blank/rnn/gru_cell/candidate/bias"]
    H = Wc.shape[1]
    h = x.new_zeros(x.shape[0], H)
    for s in range(x.shape[1]):
        g = torch.sigmoid(torch.cat([x[:, s], h], 1) @ Wg + bg)
        r, u = g.split(H, 1)
        c = torch.tanh(torch.cat([x[:, s], r * h], 1) @ Wc + bc)
        h = torch.where((lens > s)[:, None], u * h + (1 - u) * c, h)
    return h


def forward(P, batch, masks, n, rounding=True, witness=None, gates=None, capture=None):
    """P: name -> float64 leaf tensors.  Returns (total, losses dict, mid dict of tensors, tape of the routed layers)."""
    shared = PO.ln_shared_in([k for k in P])
    wit = (lambda k: witness[k]) if witness is not None else (lambda k: None)
    B, R, D = batch["image_ft"].shape
    Bn = B * n
    img, spat = _t(batch["image_ft"]), _t(batch["spatial_ft"])
    tape = {}

    def ln_act(pre, scope, i, act, site=None):
        """layer_norm over all non-batch axes of pre [B, rows, N] + activation; LayerNorm slot i (0 when shared)"""
        i = 0 if shared else i
        mu = pre.mean((1, 2), keepdim=True)
        var = pre.var((1, 2), unbiased=False, keepdim=True)
        ln = (pre - mu) * torch.rsqrt(var + O.LN_EPS) * P[PO.ln_name(scope, i) + "/gamma"] + P[PO.ln_name(scope, i) + "/beta"]
        if act == "relu" and capture is not None:
            capture[site] = (ln.detach() > 0).numpy()
        if act == "relu" and gates is not None:
            return ln * torch.as_tensor(np.asarray(gates[site]).reshape(tuple(ln.shape))).to(ln.dtype)
        return torch.relu(ln) if act == "relu" else torch.tanh(ln)

    def plain_fc(x, scope):
        return F.linear(x, P[scope + "/fc/weights"].t(), P[scope + "/fc/biases"])

    def routed_fc(x, scope):
        pre = _Routed.apply(x, P[scope + "/fc/weights"], rounding, wit(scope)) + P[scope + "/fc/biases"]
        pre.retain_grad()
        tape[scope] = (x, pre)
        return pre

    pooled, lft, valid, fills, slices = [], {}, [], [], {}
    for ki, k in enumerate(PO.KINDS):
        key = _t(batch[k + "_blank_fill/normal_boxes"])
        key6 = torch.cat([key, key[..., 2:3] - key[..., 0:1], key[..., 3:4] - key[..., 1:2]], -1)
        v = ln_act(plain_fc(spat, "spat_v_linear_v"), "spat_v_linear_v", ki, "relu", k + "/v")
        qv = ln_act(plain_fc(key6, "spat_q_linear_v"), "spat_q_linear_v", ki, "relu", k + "/qv").reshape(Bn, -1)
        feat = v.repeat_interleave(n, 0) * qv[:, None, :] * _t(masks[k + "/att"]) / O.KEEP_ATT
        s = F.linear(feat, P["spat_att/compute/score/fc/weights"].t(), P["spat_att/compute/score/fc/biases"])[..., 0]
        nbv = torch.tensor(np.repeat(np.asarray(batch["num_boxes"]), n))
        s = torch.where(torch.arange(R)[None, :] < nbv[:, None], s, torch.full_like(s, float("-inf")))
        att = torch.softmax(s, -1)
        pooled.append(torch.bmm(att[:, None, :], img.repeat_interleave(n, 0))[:, 0])                       # [Bn, D]
        valid.append(_t((np.arange(n)[None, :] < np.asarray(batch[k + "_blank_fill/num"])[:, None]).astype(np.float64)))
        fills.append(torch.tensor(np.asarray(batch[k + "_blank_fill/fills"]).astype(np.int64)))
        blanks = torch.tensor(np.asarray(batch[k + "_blank_fill/blanks"]).astype(np.int64)).reshape(Bn, -1)
        e = F.embedding(blanks, P["L_GloVe/embed_map"])
        e.retain_grad()
        slices[k + "/blank_embed"] = e
        lft[0, ki] = _gru(e, torch.tensor(np.asarray(batch[k + "_blank_fill/blanks_len"]).reshape(-1).astype(np.int64)), P)
        wse = F.embedding(torch.tensor(np.asarray(batch[k + "_blank_fill/wordsets"]).astype(np.int64)), P["wordset_map/learn"])
        wse.retain_grad()
        slices[k + "/wordset_embed"] = wse
        lft[1, ki] = ln_act(plain_fc(torch.tanh(wse), "wordset_ft"), "wordset_ft", ki, "tanh").reshape(Bn, -1)
    NH = 4
    H = lft[0, 0].shape[1]
    vl_pre = routed_fc(torch.cat(pooled, 0), "pooled_linear_l")                                            # [2 Bn, H]
    ll_pre = routed_fc(torch.cat([lft[h >> 1, h & 1] for h in range(NH)], 0), "q_linear_l")                # [NH Bn, H]
    site = lambda h, t: "%s/%s/%s" % (PO.KINDS[h & 1], HEADS[h >> 1], t)
    blk = lambda x, h, w: x[h * Bn:(h + 1) * Bn].reshape(B, n, w)
    vl = [ln_act(blk(vl_pre, h & 1, H), "pooled_linear_l", h, "relu", site(h, "vl")) for h in range(NH)]
    ll = [ln_act(blk(ll_pre, h, H), "q_linear_l", h, "relu", site(h, "ll")) for h in range(NH)]
    j_pre = routed_fc(torch.cat([(vl[h] * ll[h]).reshape(Bn, H) for h in range(NH)], 0), "joint_fc")       # [NH Bn, 2H]
    j = [ln_act(blk(j_pre, h, 2 * H), "joint_fc", h, "relu", site(h, "j")) *
         _t(masks["%s/%s_joint" % (PO.KINDS[h & 1], HEADS[h >> 1])]) / O.KEEP_JOINT for h in range(NH)]
    z = routed_fc(torch.cat([x.reshape(Bn, 2 * H) for x in j], 0), "classifier")                           # [NH Bn, A]
    losses, total = {}, 0
    for k_i, k in enumerate(PO.KINDS):       # the oracle's key (and summation) order
        for r, task in enumerate(("_blank_fill", "_wordset")):
            h = 2 * r + k_i
            ce = F.cross_entropy(z[h * Bn:(h + 1) * Bn], fills[k_i].reshape(-1), reduction="none").reshape(B, n)
            losses[k + task] = (ce * valid[k_i]).sum() / valid[k_i].sum()
    for v_ in losses.values():
        total = total + v_
    mid = {"z": z, "vl_pre": vl_pre, "ll_pre": ll_pre, "j_pre": j_pre, "pooled": torch.cat(pooled, 0)}
    return total, losses, mid, tape, slices


def loss_and_grads(p, batch, masks, n, rounding=True, witness=None, gates=None, capture=None):
    """(total loss, the four report losses, mid as numpy, grads as numpy, embedding slice grads as numpy).
    mid["z"]: the stacked logits [4 B n, A] (head h = 2 r + k); mid["routed"][layer] = {"x": left operand, "d": d_pre} of
    the four routed layers, stacked the way the step stacks them.
    witness: {layer of ROUTED: {"x": the step's left operand, "d": its d_pre}} (arrays) -- see bf16_ref._Routed; every
    entry gains "log" = {"x": ..., "d": ...}, the normalised distance of the witnessed value from this reference's own.
    gates / capture: as oracle.pretrain_oracle.torch_loss_and_grads (the ReLU sign pattern given / recorded)."""
    if witness is not None:
        assert set(witness) == set(ROUTED)
        witness = {k: {"x": _t(w["x"]), "d": _t(w["d"]), "log": w.setdefault("log", {})} for k, w in witness.items()}
    P = {k: _t(v).clone().requires_grad_(True) for k, v in p.items()}
    total, losses, mid, tape, slices = forward(P, batch, masks, n, rounding, witness, gates, capture)
    total.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    midn = {k: v.detach().numpy() for k, v in mid.items()}
    midn["routed"] = {k: {"x": tape[k][0].detach().numpy(), "d": tape[k][1].grad.numpy()} for k in ROUTED}
    return float(total.detach()), {k: float(v.detach()) for k, v in losses.items()}, midn, grads, \
        {k: v.grad.numpy() for k, v in slices.items()}


# ---- tolerances of the whole-step GPU test (tests/test_gpu_pretrain_bf16.py) against this reference in witness mode.
# Upper bounds: what tests/test_gpu_pretrain.py holds the f32 step to against the float64 oracle --
# test_forward_backward_match_oracle (its two sizes are this file's toy and medium): report scalars 2e-4 max(1, |x|),
# logits 1e-3 absolute, gradients 1e-3 max|g| + 1e-8 per tensor, the slice sum of squares 1e-3 relative;
# test_full_size_cfg5_bs512_matches_oracle_f64 (D 2048, H 1024, A 4000): the same report and logit bounds, gradients
# 5e-4 max|g| with the ReLU sign pattern of the HIP forward (gate-conditioned).
# Those bounds alone do not tell the flag on from the flag off everywhere: between the rounded and the unrounded
# reference the total loss moves by 2e-5 .. 9e-5 (the heads' losses move either way and cancel), classifier/fc/biases by
# 7e-5 .. 1.2e-3 and the toy case's gradients by 2e-3 .. 9e-3 of their max.  So each tolerance is the SMALLER of the f32
# bound and a tenth of that distance, both computed from the references alone (flag_distance; no GPU figure enters).
# "distance >= 10 x tolerance" therefore holds BY CONSTRUCTION; what can fail is that such a tolerance is too small for an
# f32 step to meet, and
# tests/test_pretrain_bf16_ref.py holds every one of them above 16 f32 ulps (1e-6) of its yardstick: the smallest is the
# total loss (1.8e-6 relative on the toy case), a mean of f32 cross-entropies that the report kernel sums in f32.
# The four per-head report losses are held at the f32 bound only: a head's loss moves by 2e-5 .. 2e-3 with the flag, so
# 2e-4 max(1, |x|) does NOT tell the flag on from the flag off for them -- that check guards the report plumbing; the
# total loss, the logits and the gradients (and the site-by-site test) carry the discrimination.
F32_REPORT_TOL = 2e-4
F32_LOGIT_TOL = 1e-3
F32_GRAD_TOL = 1e-3
F32_GRAD_TOL_GATED = 5e-4
F32_GRAD_ATOL = 1e-8
F32_SQ_TOL = 1e-3
TOL_FLOOR = 16 * 2.0 ** -24
WHOLE_STEP_CASES = (("toy", True), ("medium", True), ("medium", False), ("full_dims", True))
_DIST = {}


def grad_distance(got, want):
    """max |got - want| / max |want|: the normalised distance of a gradient tensor"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def slice_sq(slices):
    return sum(float((v ** 2).sum()) for v in slices.values())


def flag_distance(name, ln_shared=True):
    """What a step that ignored the flag would show: the distance between the rounded and the unrounded reference
    (neither witnessed) of a named case -- {"loss": relative to max(1, |loss|), "logit": absolute, "sq": relative,
    "grad/<variable>": grad_distance}.  Computed once per case."""
    key = (name, bool(ln_shared))
    if key not in _DIST:
        p, batch, masks, d = make_case(name, ln_shared)
        l0, _, m0, g0, s0 = loss_and_grads(p, batch, masks, d["n"], rounding=False)
        l1, _, m1, g1, s1 = loss_and_grads(p, batch, masks, d["n"], rounding=True)
        out = {"loss": abs(l1 - l0) / max(1.0, abs(l1)), "logit": float(np.abs(m1["z"] - m0["z"]).max()),
               "sq": abs(slice_sq(s1) - slice_sq(s0)) / slice_sq(s1)}
        for k in g1:
            if k not in PO.NO_GRAD_VARS and not k.endswith("score/fc/biases"):
                out["grad/" + k] = grad_distance(g0[k], g1[k])
        _DIST[key] = out
    return _DIST[key]


def tolerances(name, ln_shared=True):
    """{quantity of flag_distance: tolerance}: min(the f32 step's bound, a tenth of the flag's distance)"""
    gt = F32_GRAD_TOL_GATED if name == "full_dims" else F32_GRAD_TOL
    bound = lambda q: {"loss": F32_REPORT_TOL, "logit": F32_LOGIT_TOL, "sq": F32_SQ_TOL}.get(q, gt)
    return {q: min(bound(q), dist / 10) for q, dist in flag_distance(name, ln_shared).items()}
