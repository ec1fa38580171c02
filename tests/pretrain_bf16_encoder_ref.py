"""Float64 reference of the cfg-5 pre-training step with the bf16 sequence encoder (VQA_PT_FLAG_BF16_ENCODER on top of
VQA_FLAG_BF16_GEMM; PretrainEngine(precision="bf16", encoder="bf16")).

TEST INFRASTRUCTURE ONLY.  The step is tests/pretrain_bf16_ref.py's; for the duration of a call its plain-float64 caption
encoder (`_gru`) is replaced by one whose five products are rounded the way the step rounds them:
  * the packed x-projection of all steps, xp = r(x_tm) r(wx_cat) + bx_cat, with dwx = r(x_tm)^T r(dxp), dx = r(dxp) r(wx_cat)^T
    and -- row W of dwx, the constant-1 input -- bias gradients summed from ROUNDED dxp (the defined behaviour);
  * per step h r(Wg_h) and (r h) r(Wc_h) through bf16_ref._Routed: dwh = r(h)^T r(d), dh = r(d) r(W^T).
Everything else of the encoder is float64 and the state is carried unrounded.  Witnesses as bf16_ref._Routed takes them,
from the engine's named tensors ("J/x_tm", "J/hs", "J/gru_rh", "dxp", in the engine's row order); rows past their
length are not witnessed (the live recurrence does not run them and they carry no gradient)."""
from __future__ import annotations

import numpy as np
import torch

from tests import bf16_ref as BR
from tests import pretrain_bf16_ref as R

GRU_GRADS = ("encode_L_blank/rnn/gru_cell/gates/kernel", "encode_L_blank/rnn/gru_cell/candidate/kernel", "L_GloVe/embed_map")


class _RoutedX(torch.autograd.Function):
    """y = r(x) r(W) + b; dW = r(x)^T r(d); dx = r(d) r(W)^T; db = sum_rows r(d).  wit as bf16_ref._Routed."""

    @staticmethod
    def forward(ctx, x, W, b, rounding, wit):
        r = BR.round_bf16 if rounding else (lambda t: t)
        if wit is not None:
            wit["log"]["x"] = float((wit["x"] - x).abs().max() / x.abs().max().clamp_min(1e-300))
            x = wit["x"]
        xr = r(x)
        ctx.save_for_backward(xr, W)
        ctx.rounding, ctx.wit = rounding, wit
        return xr.matmul(r(W)) + b

    @staticmethod
    def backward(ctx, dy):
        xr, W = ctx.saved_tensors
        r = BR.round_bf16 if ctx.rounding else (lambda t: t)
        if ctx.wit is not None:
            ctx.wit["log"]["d"] = float((ctx.wit["d"] - dy).abs().max() / dy.abs().max().clamp_min(1e-300))
            dy = ctx.wit["d"]
        dr = r(dy)
        return dr.matmul(r(W).t()), xr.t().matmul(dr), dr.sum(0), None, None


class Encoder:
    """replacement of pretrain_bf16_ref._gru(x [rows,T,W], lens [rows], P); called once per category, object first.
    witness: None or {"x_tm" [T,2Bn,>=W], "hs" [T+1,2Bn,H], "rh" [T,2Bn,H], "dxp" [T,2Bn,3H] (float64 tensors, the
    engine's row order), "rows": LongTensor [2Bn], position of caption i (object captions first) in that order}.
    logs: every witness distance of the call."""

    def __init__(self, rounding=True, witness=None):
        self.rounding, self.witness, self.k, self.logs = rounding, witness, 0, []

    def _wit(self, own, wit_rows, d_rows, live=None):
        if self.witness is None:
            return None
        x = wit_rows if live is None else torch.where(live[:, None], wit_rows, own.detach())
        log = {}
        self.logs.append(log)
        return {"x": x, "d": d_rows, "log": log}

    def __call__(self, x, lens, P):
        Wg, bg = P["encode_L_blank/rnn/gru_cell/gates/kernel"], P["encode_L_blank/rnn/gru_cell/gates/bias"]
        Wc, bc = P["encode_L_blank/rnn/gru_cell/candidate/kernel"], P["encode_L_blank/rnn/gru_cell/candidate/bias"]
        rows, T, W = x.shape
        H = Wc.shape[1]
        w = self.witness
        idx = w["rows"][self.k * rows:(self.k + 1) * rows] if w is not None else None
        self.k += 1
        xt = x.transpose(0, 1).reshape(T * rows, W)
        wx = None
        if w is not None:
            wx = self._wit(xt, w["x_tm"][:, idx, :W].reshape(T * rows, W), w["dxp"][:, idx].reshape(T * rows, 3 * H))
        xp = _RoutedX.apply(xt, torch.cat([Wg[:W], Wc[:W]], 1), torch.cat([bg, bc]), self.rounding, wx).reshape(T, rows, 3 * H)
        h = x.new_zeros(rows, H)
        for s in range(T):
            live = lens > s
            wg = self._wit(h, w["hs"][s][idx], w["dxp"][s][idx][:, :2 * H], live) if w is not None else None
            g = torch.sigmoid(xp[s][:, :2 * H] + BR._Routed.apply(h, Wg[W:], self.rounding, wg))
            r, u = g.split(H, 1)
            rh = r * h
            wc = self._wit(rh, w["rh"][s][idx], w["dxp"][s][idx][:, 2 * H:], live) if w is not None else None
            c = torch.tanh(xp[s][:, 2 * H:] + BR._Routed.apply(rh, Wc[W:], self.rounding, wc))
            h = torch.where(live[:, None], u * h + (1 - u) * c, h)
        return h

    def witness_distance(self):
        return max([v for log in self.logs for v in log.values()], default=0.0)


def loss_and_grads(p, batch, masks, n, rounding=True, witness=None, gates=None, enc_rounding=True, enc_witness=None):
    """pretrain_bf16_ref.loss_and_grads with the caption encoder's five products rounded (enc_rounding) -- its return
    values plus the Encoder (logs).  enc_witness: see Encoder; arrays are converted."""
    if enc_witness is not None:
        enc_witness = {k: (torch.as_tensor(np.asarray(v)).long() if k == "rows" else R._t(v)) for k, v in enc_witness.items()}
    enc = Encoder(enc_rounding, enc_witness)
    keep = R._gru
    R._gru = enc
    try:
        out = R.loss_and_grads(p, batch, masks, n, rounding=rounding, witness=witness, gates=gates)
    finally:
        R._gru = keep
    return out + (enc,)


_DIST = {}


def encoder_distance(name, ln_shared=True):
    """{variable of GRU_GRADS: grad_distance between the encoder-rounded and the encoder-plain reference} (heads
    rounded in both; neither witnessed), computed once per case"""
    key = (name, bool(ln_shared))
    if key not in _DIST:
        p, batch, masks, d = R.make_case(name, ln_shared)
        g0 = loss_and_grads(p, batch, masks, d["n"], enc_rounding=False)[3]
        g1 = loss_and_grads(p, batch, masks, d["n"], enc_rounding=True)[3]
        _DIST[key] = {k: R.grad_distance(g0[k], g1[k]) for k in GRU_GRADS}
    return _DIST[key]
