"""Float64 reference of the adapted-memory pre-training model (test helper, not a test module).

vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp_adapt.py differs from the cfg-5 model
(model_vlmap_bf_or_wordset_withatt_sp.py, oracle/pretrain_oracle.py) in the memory the spatial attention pools:

    :346-350, :442-446   v_adapt = fc_layer(V_ft, V_DIM, use_ln=True, relu, scope='v_adapt') on the x n tile of image_ft;
                         layer_norm normalises over ALL non-batch axes, i.e. the whole [36, 1024] block of a row, and
                         the n tiles of an image are identical, so v_adapt is computed per image here
    :365-367, :461-463   attention_pooling(v_adapt, att_score): pooled [B, n, V_DIM], pooled_linear_l [V_DIM, V_DIM]

The scope is entered by the object and the attribute builder: one weight and bias; LayerNorm slot 0 for both (shared
reading) or slots 0 / 1 = `v_adapt/LayerNorm`, `v_adapt/LayerNorm_1` (per-call-site reading), as for the other scopes.
Everything else (scores, heads, losses, the 13 report keys) is cfg-5.

* forward: NumPy, composed from the primitives of oracle/pretrain_oracle.py.  `adapt=False` is the cfg-5 model (the
  reduction test pins it to pretrain_oracle.forward); `memory=` replaces the v_adapt layer (the mutation tests).
* torch_loss_and_grads: an independent torch restatement whose autograd gives the gradients, with the `gates=` /
  `capture=` ReLU conditioning of pretrain_oracle.torch_loss_and_grads ('<kind>/va' added to the sites).
"""
from __future__ import annotations

import numpy as np

from oracle import pretrain_oracle as PO
from oracle import vqa_oracle as O

KINDS = PO.KINDS
TOP_K = PO.TOP_K
MODEL_TYPE = "vlmap_bf_or_wordset_withatt_sp_adapt"
HEADS = ("bf", "ws")
TASK = {"bf": "blank_fill", "ws": "wordset"}


def variable_shapes(Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, adapt=True):
    """cfg-5's variables (pretrain_oracle.variable_shapes); adapt: + the v_adapt scope, pooled_linear_l [H, H]"""
    s = PO.variable_shapes(Vq, n_ws, A, W, D, H, ln_shared)
    if not adapt:
        return s
    s["pooled_linear_l/fc/weights"] = (H, H)
    s["v_adapt/fc/weights"], s["v_adapt/fc/biases"] = (D, H), (H,)
    for i in range(1 if ln_shared else 2):
        s[PO.ln_name("v_adapt", i) + "/beta"] = (H,)
        s[PO.ln_name("v_adapt", i) + "/gamma"] = (H,)
    return s


def init_params(rng, Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, adapt=True, dtype=np.float32):
    """pretrain_oracle.init_params (perturbed LayerNorms and biases), then the adapt model's own variables"""
    p = PO.init_params(rng, Vq, n_ws, A, W=W, D=D, H=H, dtype=dtype, ln_shared=ln_shared)
    if not adapt:
        return p
    for k, shp in sorted(variable_shapes(Vq, n_ws, A, W, D, H, ln_shared).items()):
        if k in p and tuple(p[k].shape) == tuple(shp):
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


def report_keys():
    return ["%s_%s_%s" % (k, TASK[h], m) for k in KINDS for h in HEADS for m in ("loss", "acc", "top_%d_acc" % TOP_K)] + \
        ["total_loss"]


def relu_sites(adapt=True):
    return PO.RELU_SITES + (tuple(k + "/va" for k in KINDS) if adapt else ())


def v_adapt(p, image_ft, ki):
    """:346-350 / :442-446 for category ki: [B, R, D] -> [B, R, H], LayerNorm over each image's [R, H] block"""
    return PO._fc_ln(image_ft, p, "v_adapt", ki, "relu")


def forward(p, batch, masks, n, adapt=True, memory=None):
    """NumPy forward: (total_loss, report, mid).  memory(p, image_ft, ki) -> the [B, R, *] block the attention pools
    (default: v_adapt with adapt, the raw features without)."""
    dt = batch["image_ft"].dtype.type
    B, R, _ = batch["image_ft"].shape
    memory = memory or (v_adapt if adapt else (lambda p_, x, ki: x))
    report, losses, mid = {}, {}, {}
    for ki, k in enumerate(KINDS):
        key = batch[k + "_blank_fill/normal_boxes"]
        key6 = np.concatenate([key, key[..., 2:3] - key[..., 0:1], key[..., 3:4] - key[..., 1:2]], -1)
        v = PO._fc_ln(batch["spatial_ft"], p, "spat_v_linear_v", ki, "relu")
        qv = PO._fc_ln(key6, p, "spat_q_linear_v", ki, "relu")
        att, _ = O.hadamard_attention_forward(np.repeat(v, n, axis=0), np.repeat(batch["num_boxes"], n),
                                              qv.reshape(B * n, -1), p["spat_att/compute/score/fc/weights"],
                                              p["spat_att/compute/score/fc/biases"], masks[k + "/att"])
        mem = memory(p, batch["image_ft"], ki)                                   # [B, R, H] (or [B, R, D])
        pooled = np.einsum("qr,qrd->qd", att, np.repeat(mem, n, axis=0)).reshape(B, n, -1)      # :365-367
        mid[k + "/att"], mid[k + "/va"], mid[k + "/pooled_V_ft"] = att, mem, pooled
        valid = (np.arange(n)[None, :] < batch[k + "_blank_fill/num"][:, None]).astype(pooled.dtype)
        fills = batch[k + "_blank_fill/fills"].astype(np.int64)
        blanks = batch[k + "_blank_fill/blanks"]
        e = p["L_GloVe/embed_map"][blanks.reshape(B * n, blanks.shape[-1])]
        g = "encode_L_blank/rnn/gru_cell/"
        bf, _ = O.gru_forward(e, batch[k + "_blank_fill/blanks_len"].reshape(-1), p[g + "gates/kernel"],
                              p[g + "gates/bias"], p[g + "candidate/kernel"], p[g + "candidate/bias"])
        wf = PO._fc_ln(np.tanh(p["wordset_map/learn"][batch[k + "_blank_fill/wordsets"]]), p, "wordset_ft", ki, "tanh")
        for r, (hd, l_ft) in enumerate((("bf", bf.reshape(B, n, -1)), ("ws", wf))):
            slot = 2 * r + ki
            vl = PO._fc_ln(pooled, p, "pooled_linear_l", slot, "relu")
            ll = PO._fc_ln(l_ft, p, "q_linear_l", slot, "relu")
            j = PO._fc_ln(vl * ll, p, "joint_fc", slot, "relu") * masks["%s/%s_joint" % (k, hd)] * dt(1.0 / O.KEEP_JOINT)
            z = j @ p["classifier/fc/weights"] + p["classifier/fc/biases"]
            mid["%s/%s_logit" % (k, hd)] = z
            name = k + "_" + TASK[hd]
            loss, acc, topk = PO.n_way_classification_loss(z, fills, valid)
            losses[name] = loss
            report[name + "_loss"], report[name + "_acc"], report[name + "_top_%d_acc" % TOP_K] = loss, acc, topk
    total = sum(losses.values())
    report["total_loss"] = total
    return total, report, mid


def torch_loss_and_grads(p, batch, masks, n, adapt=True, dtype=None, gates=None, capture=None):
    """Independent torch composition + autograd: (total_loss, per-loss values, grads, embedding slice grads) as
    pretrain_oracle.torch_loss_and_grads; gates / capture over relu_sites(adapt).  The v_adapt layer is applied to the
    x n TILE of the features as the reference does (:324-328, :346), not per image as forward() and the engine do."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in p.items()}
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    B, R, D = batch["image_ft"].shape
    img, spat = t(batch["image_ft"]), t(batch["spatial_ft"])
    shared = PO.ln_shared_in(p)

    def fc_ln(x, scope, i, act, site=None, tile=1):
        i = 0 if shared else i
        pre = F.linear(x, P[scope + "/fc/weights"].t(), P[scope + "/fc/biases"])
        dims = tuple(range(1, pre.dim()))
        mu = pre.mean(dims, keepdim=True)
        var = pre.var(dims, unbiased=False, keepdim=True)
        ln = (pre - mu) * torch.rsqrt(var + O.LN_EPS) * P[PO.ln_name(scope, i) + "/gamma"] + \
            P[PO.ln_name(scope, i) + "/beta"]
        if act == "relu" and capture is not None:
            capture[site] = (ln.detach() > 0).numpy()[::tile]          # one pattern per image (the tiles are identical)
        if act == "relu" and gates is not None:
            g = torch.as_tensor(np.asarray(gates[site])).to(dtype)
            return ln * g.reshape((-1,) + tuple(ln.shape[1:])).repeat_interleave(tile, 0)
        return torch.relu(ln) if act == "relu" else torch.tanh(ln)

    def gru(x, lens):
        g = "encode_L_blank/rnn/gru_cell/"
        Wg, bg, Wc, bc = P[g + "gates/kernel"], P[g + "gates/bias"], P[g + "candidate/kernel"], P[g + "candidate/bias"]
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
        tiled = img.repeat_interleave(n, 0)                                      # :324-328
        mem = fc_ln(tiled, "v_adapt", ki, "relu", k + "/va", tile=n) if adapt else tiled        # :346-350
        v = fc_ln(spat, "spat_v_linear_v", ki, "relu", k + "/v")
        qv = fc_ln(key6, "spat_q_linear_v", ki, "relu", k + "/qv").reshape(B * n, -1)
        feat = v.repeat_interleave(n, 0) * qv[:, None, :] * t(masks[k + "/att"]) / O.KEEP_ATT
        s = F.linear(feat, P["spat_att/compute/score/fc/weights"].t(), P["spat_att/compute/score/fc/biases"])[..., 0]
        nbv = torch.tensor(np.repeat(batch["num_boxes"], n))
        s = torch.where(torch.arange(R)[None, :] < nbv[:, None], s, torch.full_like(s, float("-inf")))
        pooled = torch.bmm(torch.softmax(s, -1)[:, None, :], mem)[:, 0].reshape(B, n, -1)       # :365-367
        valid = t((np.arange(n)[None, :] < batch[k + "_blank_fill/num"][:, None]).astype(np.float64))
        fills = torch.tensor(batch[k + "_blank_fill/fills"].astype(np.int64))
        blanks = torch.tensor(batch[k + "_blank_fill/blanks"].astype(np.int64)).reshape(B * n, -1)
        e = F.embedding(blanks, P["L_GloVe/embed_map"])
        e.retain_grad()
        slices[k + "/blank_embed"] = e
        bf = gru(e, torch.tensor(batch[k + "_blank_fill/blanks_len"].reshape(-1).astype(np.int64))).reshape(B, n, -1)
        wse = F.embedding(torch.tensor(batch[k + "_blank_fill/wordsets"].astype(np.int64)), P["wordset_map/learn"])
        wse.retain_grad()
        slices[k + "/wordset_embed"] = wse
        wf = fc_ln(torch.tanh(wse), "wordset_ft", ki, "tanh")
        for r, (hd, l_ft) in enumerate((("bf", bf), ("ws", wf))):
            slot, site = 2 * r + ki, "%s/%s/" % (k, hd)
            vl = fc_ln(pooled, "pooled_linear_l", slot, "relu", site + "vl")
            ll = fc_ln(l_ft, "q_linear_l", slot, "relu", site + "ll")
            j = fc_ln(vl * ll, "joint_fc", slot, "relu", site + "j") * t(masks["%s/%s_joint" % (k, hd)]) / O.KEEP_JOINT
            z = F.linear(j, P["classifier/fc/weights"].t(), P["classifier/fc/biases"])
            c = F.cross_entropy(z.reshape(B * n, -1), fills.reshape(-1), reduction="none").reshape(B, n)
            losses[k + "_" + TASK[hd]] = (c * valid).sum() / valid.sum()
    total = 0
    for vloss in losses.values():
        total = total + vloss
    total.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in P.items()}
    return float(total.detach()), {k: float(v.detach()) for k, v in losses.items()}, grads, \
        {k: v.grad.numpy() for k, v in slices.items()}
