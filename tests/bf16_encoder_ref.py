"""Float64 reference of the bf16 VQA step with the question encoder's single products routed (VQA_FLAG_BF16_ENCODER_GEMMS on
top of VQA_FLAG_BF16_GEMM; FusionEngine(precision="bf16", encoder="bf16-gemms")).

TEST INFRASTRUCTURE ONLY.  The step is tests/bf16_ref.py's; for the duration of a call its plain-float64 question encoder
(`_gru`) is replaced by one whose five single products are rounded the way the step rounds them and whose recurrence is not:
  * the packed x-projection of all steps through pretrain_bf16_encoder_ref._RoutedX: xp = r(x_tm) r(wx_cat) + bx_cat,
    dwx = r(x_tm)^T r(dxp), dx = r(dxp) r(wx_cat)^T and -- row W of dwx, the constant-1 input -- bias gradients summed from
    ROUNDED dxp (the defined behaviour of the packed form);
  * per step the recurrent products h Wg_h and (r h) Wc_h through _RecurrentW: forward h W PLAIN, dh = d W^T PLAIN (both
    belong to the recurrence, which stays f32), dW = r(h)^T r(d) (the dwh GEMM).
The state is carried unrounded.  Witnesses as bf16_ref._Routed takes them, from the engine's tensors dxp, hs and gru_rh
(time-major, the engine's row order = the batch's); x_tm and the weights are inputs and never witnessed; rows past their
length are not witnessed (the live recurrence does not write them and they carry no gradient)."""
from __future__ import annotations

import numpy as np
import torch

from oracle import vqa_oracle as O
from tests import bf16_ref as R
from tests.pretrain_bf16_encoder_ref import _RoutedX


def gru_names(model_type):
    """the four GRU variables of the model type: gate kernel, gate bias, candidate kernel, candidate bias"""
    sc = O.scope_names(model_type)
    return (sc["gru_gates"] + "/kernel", sc["gru_gates"] + "/bias", sc["gru_cand"] + "/kernel", sc["gru_cand"] + "/bias")


class _RecurrentW(torch.autograd.Function):
    """y = h W and dh = d W^T unrounded (the recurrence); dW = r(h)^T r(d) (the dwh GEMM).  wit: {"x": the step's own h,
    "d": its own dxp columns, "log": dict} -- used for dW only, after logging their distance from this reference's own."""

    @staticmethod
    def forward(ctx, h, W, rounding, wit):
        ctx.save_for_backward(h, W)
        ctx.rounding, ctx.wit = rounding, wit
        return h.matmul(W)

    @staticmethod
    def backward(ctx, dy):
        h, W = ctx.saved_tensors
        r = R.round_bf16 if ctx.rounding else (lambda t: t)
        hw, dw = h, dy
        if ctx.wit is not None:
            hw, dw = ctx.wit["x"], ctx.wit["d"]
            ctx.wit["log"]["x"] = float((hw - h).abs().max() / h.abs().max().clamp_min(1e-300))
            ctx.wit["log"]["d"] = float((dw - dy).abs().max() / dy.abs().max().clamp_min(1e-300))
        return dy.matmul(W.t()), r(hw).t().matmul(r(dw)), None, None


class Encoder:
    """replacement of bf16_ref._gru(x [B,T,W], lens [B], Wg, bg, Wc, bc).  witness: None or {"hs" [T+1,B,H], "rh" [T,B,H],
    "dxp" [T,B,3H]} (float64 tensors).  logs: every witness distance of the call.  tape(): this reference's own hs, rh and
    (after the backward) dxp, the tensors a witness stands in for."""

    def __init__(self, rounding=True, witness=None):
        self.rounding, self.witness, self.logs = rounding, witness, []

    def _wit(self, x, d):
        log = {}
        self.logs.append(log)
        return {"x": x, "d": d, "log": log}

    def __call__(self, x, lens, Wg, bg, Wc, bc):
        B, T, W = x.shape
        H = Wc.shape[1]
        w = self.witness
        xt = x.transpose(0, 1).reshape(T * B, W)
        live_all = (lens[None, :] > torch.arange(T)[:, None])                                   # [T,B]
        zero = x.new_zeros(())
        wx = None
        if w is not None:      # x_tm is an input: its own value stands in; dxp of a finished row is zero on both sides
            wx = self._wit(xt.detach(), torch.where(live_all[:, :, None], w["dxp"], zero).reshape(T * B, 3 * H))
        xp = _RoutedX.apply(xt, torch.cat([Wg[:W], Wc[:W]], 1), torch.cat([bg, bc]), self.rounding, wx).reshape(T, B, 3 * H)
        xp.retain_grad()
        h = x.new_zeros(B, H)
        self._xp, self._hs, self._rh = xp, [h], []
        for s in range(T):
            live = live_all[s][:, None]
            wg = wc = None
            if w is not None:
                d = torch.where(live, w["dxp"][s], zero)
                wg = self._wit(torch.where(live, w["hs"][s], h.detach()), d[:, :2 * H])
            g = torch.sigmoid(xp[s][:, :2 * H] + _RecurrentW.apply(h, Wg[W:], self.rounding, wg))
            r, u = g.split(H, 1)
            rh = r * h
            if w is not None:
                wc = self._wit(torch.where(live, w["rh"][s], rh.detach()), d[:, 2 * H:])
            c = torch.tanh(xp[s][:, 2 * H:] + _RecurrentW.apply(rh, Wc[W:], self.rounding, wc))
            h = torch.where(live, u * h + (1 - u) * c, h)
            self._hs.append(h.detach())
            self._rh.append(rh.detach())
        return h

    def tape(self):
        return {"hs": torch.stack(self._hs).numpy(), "rh": torch.stack(self._rh).numpy(), "dxp": self._xp.grad.numpy()}

    def witness_distance(self):
        return max([v for log in self.logs for v in log.values()], default=0.0)


def loss_and_grads(params, batch, table, nbox_table, answer_masks, masks, model_type="vlmap_answer", rounding=True,
                   witness=None, enc_rounding=True, enc_witness=None):
    """bf16_ref.loss_and_grads with the question encoder's five single products rounded (enc_rounding) -- its return values
    plus the Encoder (logs).  enc_witness: see Encoder; arrays are converted."""
    if enc_witness is not None:
        enc_witness = {k: R._t(np.asarray(v)) for k, v in enc_witness.items()}
    enc = Encoder(enc_rounding, enc_witness)
    keep = R._gru
    R._gru = enc
    try:
        out = R.loss_and_grads(params, batch, table, nbox_table, answer_masks, masks, model_type, rounding=rounding,
                               witness=witness)
    finally:
        R._gru = keep
    return out + (enc,)


_CASES = {}


def reference_pair(model_type, case):
    """(encoder-plain, encoder-rounded) unwitnessed references of a model case (dense layers rounded in both), computed
    once per (model type, case) and never changed"""
    from tests.gpu_util import make_case
    name, dims, B, Rg, T, N = case
    key = (model_type, name, B)
    if key not in _CASES:
        p, table, nbox, batch, am, masks = make_case(R.MODEL_SEED, model_type, B, Rg, T, N, dims)
        pp = {k: v for k, v in p.items() if not O.is_const(k)}
        _CASES[key] = tuple(loss_and_grads(pp, batch, table, nbox, am, masks, model_type, enc_rounding=e)[:5] for e in (False, True))
    return _CASES[key]
