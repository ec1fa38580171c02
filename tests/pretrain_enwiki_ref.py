"""Float64 reference of the pre-training models with a variable head set (test helper, not a test module).

vlmap_memft/model_vlmap_bf_or_wordset_enwiki_withatt_sp.py is the cfg-5 model of oracle/pretrain_oracle.py plus, per
category, build_*_enwiki (:519-624): enwiki_map embedding of the answer's Wikipedia context [B, n, Lc] -> encode_L
(scope 'encode_L_enwiki', GRU, lengths enwiki_context_len, shared by both categories) -> the shared pooled_linear_l,
q_linear_l, joint_fc (dropout 0.5) and classifier -> the masked softmax-CE over the blank-fill fills.
model_vlmap_bf_enwiki_withatt_sp.py drops the word-set heads (:83-84).  Heads are built in the order bf, ws, ew, object
before attribute, so head 2 r + k (type of rank r, category k) owns LayerNorm slot 2 r + k of the shared fusion scopes
when they are not shared (`LayerNorm` ... `LayerNorm_5`).

* forward: NumPy, composed from the oracle's primitives (pretrain_oracle._fc_ln / n_way_classification_loss,
  vqa_oracle.gru_forward / hadamard_attention_forward), the same way pretrain_oracle.forward composes them.
* torch_loss_and_grads: an independent torch restatement whose autograd gives the gradients, with the `gates=` /
  `capture=` ReLU conditioning of pretrain_oracle.torch_loss_and_grads.
With heads ("bf", "ws") both reduce to pretrain_oracle's forward / torch_loss_and_grads.
"""
from __future__ import annotations

import numpy as np

from oracle import pretrain_oracle as PO
from oracle import vqa_oracle as O

KINDS = PO.KINDS
TOP_K = PO.TOP_K
HEADS_ALL = ("bf", "ws", "ew")
TASK = {"bf": "blank_fill", "ws": "wordset", "ew": "enwiki"}
GRU_VARS = ("gates/kernel", "gates/bias", "candidate/kernel", "candidate/bias")


def ln_slots(heads):
    return 2 * len(heads)


def variable_shapes(Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, heads=HEADS_ALL, n_ctx=None):
    """pretrain_oracle.variable_shapes for a head set (stated independently of the engine's)."""
    s = {"wordset_map/learn": (n_ws, W), "V_GloVe/embed_map": (Vq, W), "L_GloVe/embed_map": (Vq, W),
         "LearnAnswerGloVe/embed_map": (A, W)}
    if "ew" in heads:
        s["enwiki_map/learn"] = (n_ctx, W)

    def fc(scope, fin, fout, n_ln):
        s[scope + "/fc/weights"] = (fin, fout)
        s[scope + "/fc/biases"] = (fout,)
        for i in range(min(n_ln, 1) if ln_shared else n_ln):
            s[PO.ln_name(scope, i) + "/beta"] = (fout,)
            s[PO.ln_name(scope, i) + "/gamma"] = (fout,)

    fc("spat_v_linear_v", 6, H, 2)
    fc("spat_q_linear_v", 6, H, 2)
    fc("spat_att/compute/score", H, 1, 0)
    for scope in ("encode_L_blank",) + (("encode_L_enwiki",) if "ew" in heads else ()):
        s[scope + "/rnn/gru_cell/gates/kernel"] = (W + H, 2 * H)
        s[scope + "/rnn/gru_cell/gates/bias"] = (2 * H,)
        s[scope + "/rnn/gru_cell/candidate/kernel"] = (W + H, H)
        s[scope + "/rnn/gru_cell/candidate/bias"] = (H,)
    fc("pooled_linear_l", D, H, ln_slots(heads))
    fc("q_linear_l", H, H, ln_slots(heads))
    fc("joint_fc", H, 2 * H, ln_slots(heads))
    if "ws" in heads:
        fc("wordset_ft", W, H, 2)
    fc("classifier", 2 * H, A, 0)
    return s


def init_params(rng, Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, heads=HEADS_ALL, n_ctx=None,
                dtype=np.float32):
    """pretrain_oracle.init_params (perturbed LayerNorms and biases) for a head set: the cfg-5 variables first, drawn
    exactly as there, then the enwiki ones."""
    p = PO.init_params(rng, Vq, n_ws, A, W=W, D=D, H=H, ln_shared=ln_shared, dtype=dtype)
    want = variable_shapes(Vq, n_ws, A, W, D, H, ln_shared, heads, n_ctx)
    for k in list(p):
        if k not in want:
            del p[k]
    for k, shp in want.items():
        if k in p:
            continue
        if k.endswith("/kernel"):
            lim = np.sqrt(6.0 / (shp[0] + shp[1]))
            v = rng.uniform(-lim, lim, size=shp)
        elif k.endswith("gates/bias"):
            v = np.ones(shp) + 0.1 * rng.standard_normal(shp)
        elif k.endswith("/learn"):
            v = rng.uniform(-0.01, 0.01, size=shp)
        elif k.endswith("/gamma"):
            v = np.ones(shp) + 0.1 * rng.standard_normal(shp)
        else:
            v = 0.1 * rng.standard_normal(shp)
        p[k] = v.astype(dtype)
    return p


def add_enwiki_fields(rng, batch, n_ctx, Lc):
    """{kind}_blank_fill/enwiki_context [B,n,Lc] (zero padded, tokens 1 .. n_ctx-1) and _len [B,n] in 1 .. Lc"""
    B, n = batch["obj_blank_fill/fills"].shape
    for k in KINDS:
        lens = rng.integers(1, Lc + 1, size=(B, n)).astype(np.int32)
        ctx = rng.integers(1, n_ctx, size=(B, n, Lc)).astype(np.int32)
        ctx[np.arange(Lc)[None, None, :] >= lens[..., None]] = 0
        batch[k + "_blank_fill/enwiki_context"], batch[k + "_blank_fill/enwiki_context_len"] = ctx, lens
    return batch


def add_enwiki_masks(rng, masks, B, n, H, dtype=np.float32):
    for k in KINDS:
        masks[k + "/ew_joint"] = (rng.random((B, n, 2 * H)) < O.KEEP_JOINT).astype(dtype)
    return masks


def report_keys(heads):
    return ["%s_%s_%s" % (k, TASK[h], m) for k in KINDS for h in heads
            for m in ("loss", "acc", "top_%d_acc" % TOP_K)] + ["total_loss"]


def relu_sites(heads):
    return tuple("%s/%s" % (k, s) for k in KINDS for s in ("v", "qv") + tuple(
        "%s/%s" % (h, t) for h in heads for t in ("vl", "ll", "j")))


def _gru_np(p, scope, x, lens):
    g = scope + "/rnn/gru_cell/"
    h, _ = O.gru_forward(x, lens, p[g + "gates/kernel"], p[g + "gates/bias"], p[g + "candidate/kernel"],
                         p[g + "candidate/bias"])
    return h


def forward(p, batch, masks, n, heads=HEADS_ALL):
    """NumPy float64 forward: (total_loss, report, mid) with mid['<kind>/<head>_logit'], '<kind>/att'."""
    dt = batch["image_ft"].dtype.type
    B, R, D = batch["image_ft"].shape
    report, losses, mid = {}, {}, {}
    for ki, k in enumerate(KINDS):
        key = batch[k + "_blank_fill/normal_boxes"]
        key6 = np.concatenate([key, key[..., 2:3] - key[..., 0:1], key[..., 3:4] - key[..., 1:2]], -1)
        v = PO._fc_ln(batch["spatial_ft"], p, "spat_v_linear_v", ki, "relu")
        qv = PO._fc_ln(key6, p, "spat_q_linear_v", ki, "relu")
        att, _ = O.hadamard_attention_forward(np.repeat(v, n, axis=0), np.repeat(batch["num_boxes"], n),
                                              qv.reshape(B * n, -1), p["spat_att/compute/score/fc/weights"],
                                              p["spat_att/compute/score/fc/biases"], masks[k + "/att"])
        pooled = np.einsum("qr,qrd->qd", att, np.repeat(batch["image_ft"], n, axis=0)).reshape(B, n, D)
        mid[k + "/att"] = att
        valid = (np.arange(n)[None, :] < batch[k + "_blank_fill/num"][:, None]).astype(pooled.dtype)
        fills = batch[k + "_blank_fill/fills"].astype(np.int64)
        for r, hd in enumerate(heads):
            slot = 2 * r + ki
            if hd == "bf":
                blanks = batch[k + "_blank_fill/blanks"]
                e = p["L_GloVe/embed_map"][blanks.reshape(B * n, blanks.shape[-1])]
                l_ft = _gru_np(p, "encode_L_blank", e, batch[k + "_blank_fill/blanks_len"].reshape(-1)).reshape(B, n, -1)
            elif hd == "ws":
                ws = np.tanh(p["wordset_map/learn"][batch[k + "_blank_fill/wordsets"]])
                l_ft = PO._fc_ln(ws, p, "wordset_ft", ki, "tanh")
            else:
                ctx = batch[k + "_blank_fill/enwiki_context"]
                e = p["enwiki_map/learn"][ctx.reshape(B * n, ctx.shape[-1])]
                l_ft = _gru_np(p, "encode_L_enwiki", e,
                               batch[k + "_blank_fill/enwiki_context_len"].reshape(-1)).reshape(B, n, -1)
            vl = PO._fc_ln(pooled, p, "pooled_linear_l", slot, "relu")
            ll = PO._fc_ln(l_ft, p, "q_linear_l", slot, "relu")
            j = PO._fc_ln(vl * ll, p, "joint_fc", slot, "relu") * masks["%s/%s_joint" % (k, hd)] * dt(1.0 / O.KEEP_JOINT)
            logit = j @ p["classifier/fc/weights"] + p["classifier/fc/biases"]
            loss, acc, topk = PO.n_way_classification_loss(logit, fills, valid)
            t = TASK[hd]
            losses[k + "_" + t] = loss
            report[k + "_%s_loss" % t], report[k + "_%s_acc" % t] = loss, acc
            report[k + "_%s_top_%d_acc" % (t, TOP_K)] = topk
            mid["%s/%s_logit" % (k, hd)] = logit
    total = sum(losses.values())
    report["total_loss"] = total
    return total, report, mid


def torch_loss_and_grads(p, batch, masks, n, heads=HEADS_ALL, dtype=None, gates=None, capture=None):
    """Independent torch composition + autograd: (total_loss, per-head losses, grads, embedding slice grads) as
    pretrain_oracle.torch_loss_and_grads; gates / capture over relu_sites(heads)."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in p.items()}
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    B, R, D = batch["image_ft"].shape
    img, spat = t(batch["image_ft"]), t(batch["spatial_ft"])
    shared = PO.ln_shared_in(p)

    def fc_ln(x, scope, i, act, site=None):
        i = 0 if shared else i
        pre = F.linear(x, P[scope + "/fc/weights"].t(), P[scope + "/fc/biases"])
        dims = tuple(range(1, pre.dim()))
        mu = pre.mean(dims, keepdim=True)
        var = pre.var(dims, unbiased=False, keepdim=True)
        ln = (pre - mu) * torch.rsqrt(var + O.LN_EPS) * P[PO.ln_name(scope, i) + "/gamma"] + \
            P[PO.ln_name(scope, i) + "/beta"]
        if act == "relu" and capture is not None:
            capture[site] = (ln.detach() > 0).numpy()
        if act == "relu" and gates is not None:
            return ln * torch.as_tensor(np.asarray(gates[site]).reshape(tuple(ln.shape))).to(dtype)
        return torch.relu(ln) if act == "relu" else torch.tanh(ln)

    def gru(scope, x, lens):
        g = scope + "/rnn/gru_cell/"
        Wg, bg, Wc, bc = (P[g + v] for v in GRU_VARS)
        H = Wc.shape[1]
        h = x.new_zeros(x.shape[0], H)
        for s in range(x.shape[1]):
            gg = torch.sigmoid(torch.cat([x[:, s], h], 1) @ Wg + bg)
            r, u = gg.split(H, 1)
            c = torch.tanh(torch.cat([x[:, s], r * h], 1) @ Wc + bc)
            h = torch.where((lens > s)[:, None], u * h + (1 - u) * c, h)
        return h

    losses, slices = {}, {}
    for ki, k in enumerate(KINDS):
        key = t(batch[k + "_blank_fill/normal_boxes"])
        key6 = torch.cat([key, key[..., 2:3] - key[..., 0:1], key[..., 3:4] - key[..., 1:2]], -1)
        v = fc_ln(spat, "spat_v_linear_v", ki, "relu", k + "/v")
        qv = fc_ln(key6, "spat_q_linear_v", ki, "relu", k + "/qv").reshape(B * n, -1)
        feat = v.repeat_interleave(n, 0) * qv[:, None, :] * t(masks[k + "/att"]) / O.KEEP_ATT
        s = F.linear(feat, P["spat_att/compute/score/fc/weights"].t(), P["spat_att/compute/score/fc/biases"])[..., 0]
        nbv = torch.tensor(np.repeat(batch["num_boxes"], n))
        s = torch.where(torch.arange(R)[None, :] < nbv[:, None], s, torch.full_like(s, float("-inf")))
        pooled = torch.bmm(torch.softmax(s, -1)[:, None, :], img.repeat_interleave(n, 0))[:, 0].reshape(B, n, D)
        valid = t((np.arange(n)[None, :] < batch[k + "_blank_fill/num"][:, None]).astype(np.float64))
        fills = torch.tensor(batch[k + "_blank_fill/fills"].astype(np.int64))
        for r, hd in enumerate(heads):
            slot = 2 * r + ki
            if hd == "bf":
                blanks = torch.tensor(batch[k + "_blank_fill/blanks"].astype(np.int64)).reshape(B * n, -1)
                e = F.embedding(blanks, P["L_GloVe/embed_map"])
                e.retain_grad()
                slices[k + "/blank_embed"] = e
                lens = torch.tensor(batch[k + "_blank_fill/blanks_len"].reshape(-1).astype(np.int64))
                l_ft = gru("encode_L_blank", e, lens).reshape(B, n, -1)
            elif hd == "ws":
                wse = F.embedding(torch.tensor(batch[k + "_blank_fill/wordsets"].astype(np.int64)), P["wordset_map/learn"])
                wse.retain_grad()
                slices[k + "/wordset_embed"] = wse
                l_ft = fc_ln(torch.tanh(wse), "wordset_ft", ki, "tanh")
            else:
                ctx = torch.tensor(batch[k + "_blank_fill/enwiki_context"].astype(np.int64)).reshape(B * n, -1)
                e = F.embedding(ctx, P["enwiki_map/learn"])
                e.retain_grad()
                slices[k + "/enwiki_embed"] = e
                lens = torch.tensor(batch[k + "_blank_fill/enwiki_context_len"].reshape(-1).astype(np.int64))
                l_ft = gru("encode_L_enwiki", e, lens).reshape(B, n, -1)
            site = "%s/%s/" % (k, hd)
            vl = fc_ln(pooled, "pooled_linear_l", slot, "relu", site + "vl")
            ll = fc_ln(l_ft, "q_linear_l", slot, "relu", site + "ll")
            j = fc_ln(vl * ll, "joint_fc", slot, "relu", site + "j") * t(masks["%s/%s_joint" % (k, hd)]) / O.KEEP_JOINT
            z = F.linear(j, P["classifier/fc/weights"].t(), P["classifier/fc/biases"])
            ce = F.cross_entropy(z.reshape(B * n, -1), fills.reshape(-1), reduction="none").reshape(B, n)
            losses[k + "_" + TASK[hd]] = (ce * valid).sum() / valid.sum()
    total = 0
    for vloss in losses.values():
        total = total + vloss
    total.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    return float(total.detach()), {k: float(v.detach()) for k, v in losses.items()}, grads, \
        {k: v.grad.numpy() for k, v in slices.items()}
