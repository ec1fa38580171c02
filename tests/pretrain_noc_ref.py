"""Float64 reference of the "no composition" pre-training models (test helper, not a test module).

vlmap_memft/model_vlmap_noc_bf_or_wordset_withatt_sp.py (= model_vlmap_nocarch_bf_or_wordset_withatt_sp.py, heads bf, ws)
and model_vlmap_noc_bf_or_enwiki_withatt_sp.py (bf, ew) share everything up to v_linear_l (pooled_linear_l) and l_linear_l
(q_linear_l) with the models of tests/pretrain_enwiki_ref.py.  After that, per head, there is no Hadamard product:

    v_joint = dropout(relu(LN(v_linear_l @ joint_v + b)), 0.5)     l_joint = dropout(relu(LN(l_linear_l @ joint_l + b)), 0.5)
    v_logit = v_joint @ classifier_v + b                           l_logit = l_joint @ classifier_l + b

A blank-fill head (SUM) has one masked softmax-CE of v_logit + l_logit; a word-set / enwiki head (SPLIT) has one of
v_logit and one of l_logit.  The total is the sum of all six losses.  Head h = 2 r + k owns LayerNorm slot h of
pooled_linear_l, q_linear_l, joint_v and joint_l when they are not shared.

* forward: NumPy, composed from the primitives of oracle/pretrain_oracle.py and tests/pretrain_enwiki_ref.py.
* torch_loss_and_grads: an independent torch restatement whose autograd gives the gradients, with the `gates=` /
  `capture=` ReLU conditioning of pretrain_oracle.torch_loss_and_grads.
"""
from __future__ import annotations

import numpy as np

from oracle import pretrain_oracle as PO
from oracle import vqa_oracle as O
from tests import pretrain_enwiki_ref as ER

KINDS = PO.KINDS
TOP_K = PO.TOP_K
TASK = ER.TASK
TYPES = {"vlmap_noc_bf_or_wordset_withatt_sp": ("bf", "ws"), "vlmap_nocarch_bf_or_wordset_withatt_sp": ("bf", "ws"),
         "vlmap_noc_bf_or_enwiki_withatt_sp": ("bf", "ew")}
SPLIT = {"bf": False, "ws": True, "ew": True}


def variable_shapes(Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, heads=("bf", "ws"), n_ctx=None):
    """the head set's variables (pretrain_enwiki_ref.variable_shapes) with joint_fc -> joint_v, joint_l and
    classifier -> classifier_v, classifier_l"""
    s = ER.variable_shapes(Vq, n_ws, A, W, D, H, ln_shared, heads, n_ctx)
    out = {}
    for k, v in s.items():
        scope = k.split("/")[0]
        if scope in ("joint_fc", "classifier"):
            for br in ("v", "l"):
                out[k.replace(scope, "%s_%s" % ("joint" if scope == "joint_fc" else scope, br), 1)] = v
        else:
            out[k] = v
    return out


def init_params(rng, Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, heads=("bf", "ws"), n_ctx=None,
                dtype=np.float32):
    """pretrain_enwiki_ref.init_params (perturbed LayerNorms and biases) for the trunk, then the two branches' scopes"""
    p = ER.init_params(rng, Vq, n_ws, A, W=W, D=D, H=H, ln_shared=ln_shared, heads=heads, n_ctx=n_ctx, dtype=dtype)
    for k in [k for k in p if k.split("/")[0] in ("joint_fc", "classifier")]:
        del p[k]
    for k, shp in sorted(variable_shapes(Vq, n_ws, A, W, D, H, ln_shared, heads, n_ctx).items()):
        if k in p:
            continue
        if k.endswith("/weights"):
            lim = np.sqrt(6.0 / (shp[0] + shp[1]))
            v = rng.uniform(-lim, lim, size=shp)
        elif k.endswith("/gamma"):
            v = np.ones(shp) + 0.1 * rng.standard_normal(shp)
        else:
            v = 0.1 * rng.standard_normal(shp)
        p[k] = v.astype(dtype)
    return p


def add_noc_masks(rng, masks, B, n, H, heads, dtype=np.float32):
    """the l branch's keep-masks '<kind>/<head>_joint_l'; the v branch uses '<kind>/<head>_joint'"""
    for k in KINDS:
        for h in heads:
            masks["%s/%s_joint_l" % (k, h)] = (rng.random((B, n, 2 * H)) < O.KEEP_JOINT).astype(dtype)
    return masks


def report_keys(heads):
    return ["%s_%s%s_%s" % (k, TASK[h], b, m) for k in KINDS for h in heads
            for b in (("_v", "_l") if SPLIT[h] else ("",)) for m in ("loss", "acc", "top_%d_acc" % TOP_K)] + \
        ["total_loss"]


def relu_sites(heads):
    return tuple("%s/%s" % (k, s) for k in KINDS for s in ("v", "qv") + tuple(
        "%s/%s" % (h, t) for h in heads for t in ("vl", "ll", "jv", "jl")))


def trunk(p, batch, masks, n, heads):
    """pooled V features and each head's language feature l_ft (bf_state / wf / ew_state) per category"""
    B, R, D = batch["image_ft"].shape
    out = {}
    for ki, k in enumerate(KINDS):
        key = batch[k + "_blank_fill/normal_boxes"]
        key6 = np.concatenate([key, key[..., 2:3] - key[..., 0:1], key[..., 3:4] - key[..., 1:2]], -1)
        v = PO._fc_ln(batch["spatial_ft"], p, "spat_v_linear_v", ki, "relu")
        qv = PO._fc_ln(key6, p, "spat_q_linear_v", ki, "relu")
        att, _ = O.hadamard_attention_forward(np.repeat(v, n, axis=0), np.repeat(batch["num_boxes"], n),
                                              qv.reshape(B * n, -1), p["spat_att/compute/score/fc/weights"],
                                              p["spat_att/compute/score/fc/biases"], masks[k + "/att"])
        out[k + "/att"] = att
        out[k + "/pooled"] = np.einsum("qr,qrd->qd", att, np.repeat(batch["image_ft"], n, axis=0)).reshape(B, n, D)
        for hd in heads:
            if hd == "bf":
                blanks = batch[k + "_blank_fill/blanks"]
                e = p["L_GloVe/embed_map"][blanks.reshape(B * n, blanks.shape[-1])]
                l_ft = ER._gru_np(p, "encode_L_blank", e, batch[k + "_blank_fill/blanks_len"].reshape(-1))
                out[k + "/bf_state"] = l_ft.reshape(B, n, -1)
            elif hd == "ws":
                ws = np.tanh(p["wordset_map/learn"][batch[k + "_blank_fill/wordsets"]])
                out[k + "/wf"] = PO._fc_ln(ws, p, "wordset_ft", ki, "tanh")
            else:
                ctx = batch[k + "_blank_fill/enwiki_context"]
                e = p["enwiki_map/learn"][ctx.reshape(B * n, ctx.shape[-1])]
                l_ft = ER._gru_np(p, "encode_L_enwiki", e, batch[k + "_blank_fill/enwiki_context_len"].reshape(-1))
                out[k + "/ew_state"] = l_ft.reshape(B, n, -1)
    return out


STATE = {"bf": "bf_state", "ws": "wf", "ew": "ew_state"}


def forward(p, batch, masks, n, heads=("bf", "ws"), ce=None):
    """NumPy float64 forward: (total_loss, report, mid) with mid['<kind>/<head>_zv' | '_zl'] and the trunk's tensors.
    ce: the masked softmax-CE (default pretrain_oracle.n_way_classification_loss)."""
    ce = ce or PO.n_way_classification_loss
    dt = batch["image_ft"].dtype.type
    mid = trunk(p, batch, masks, n, heads)
    report, losses = {}, {}
    for ki, k in enumerate(KINDS):
        valid = (np.arange(n)[None, :] < batch[k + "_blank_fill/num"][:, None]).astype(mid[k + "/pooled"].dtype)
        fills = batch[k + "_blank_fill/fills"].astype(np.int64)
        for r, hd in enumerate(heads):
            slot = 2 * r + ki
            vl = PO._fc_ln(mid[k + "/pooled"], p, "pooled_linear_l", slot, "relu")
            ll = PO._fc_ln(mid[k + "/" + STATE[hd]], p, "q_linear_l", slot, "relu")
            jv = PO._fc_ln(vl, p, "joint_v", slot, "relu") * masks["%s/%s_joint" % (k, hd)] * dt(1.0 / O.KEEP_JOINT)
            jl = PO._fc_ln(ll, p, "joint_l", slot, "relu") * masks["%s/%s_joint_l" % (k, hd)] * dt(1.0 / O.KEEP_JOINT)
            zv = jv @ p["classifier_v/fc/weights"] + p["classifier_v/fc/biases"]
            zl = jl @ p["classifier_l/fc/weights"] + p["classifier_l/fc/biases"]
            mid["%s/%s_zv" % (k, hd)], mid["%s/%s_zl" % (k, hd)] = zv, zl
            t = k + "_" + TASK[hd]
            parts = ((t + "_v", zv), (t + "_l", zl)) if SPLIT[hd] else ((t, zv + zl),)
            for name, z in parts:
                loss, acc, topk = ce(z, fills, valid)
                losses[name] = loss
                report[name + "_loss"], report[name + "_acc"] = loss, acc
                report[name + "_top_%d_acc" % TOP_K] = topk
    total = sum(losses.values())
    report["total_loss"] = total
    return total, report, mid


def torch_loss_and_grads(p, batch, masks, n, heads=("bf", "ws"), dtype=None, gates=None, capture=None):
    """Independent torch composition + autograd: (total_loss, per-loss values, grads, embedding slice grads) as
    pretrain_enwiki_ref.torch_loss_and_grads; gates / capture over relu_sites(heads)."""
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
        Wg, bg, Wc, bc = (P[g + v] for v in ER.GRU_VARS)
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
            jv = fc_ln(vl, "joint_v", slot, "relu", site + "jv") * t(masks["%s/%s_joint" % (k, hd)]) / O.KEEP_JOINT
            jl = fc_ln(ll, "joint_l", slot, "relu", site + "jl") * t(masks["%s/%s_joint_l" % (k, hd)]) / O.KEEP_JOINT
            zv = F.linear(jv, P["classifier_v/fc/weights"].t(), P["classifier_v/fc/biases"])
            zl = F.linear(jl, P["classifier_l/fc/weights"].t(), P["classifier_l/fc/biases"])
            name = k + "_" + TASK[hd]
            parts = ((name + "_v", zv), (name + "_l", zl)) if SPLIT[hd] else ((name, zv + zl),)
            for nm, z in parts:
                c = F.cross_entropy(z.reshape(B * n, -1), fills.reshape(-1), reduction="none").reshape(B, n)
                losses[nm] = (c * valid).sum() / valid.sum()
    total = 0
    for vloss in losses.values():
        total = total + vloss
    total.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    return float(total.detach()), {k: float(v.detach()) for k, v in losses.items()}, grads, \
        {k: v.grad.numpy() for k, v in slices.items()}
