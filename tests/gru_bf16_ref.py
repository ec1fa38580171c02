"""Float64 reference of the GRU recurrence with bf16 operands in its two recurrent products (csrc/gru_step_bf16.hip:
GRU-step id 64, VQA_PT_FLAG_BF16_ENCODER) and the comparators of the op-level tests.

The recurrence is tests/gru_ref.py's (forward / backward with a `step=` cell); the cell sends its two products through
tests.bf16_ref._Routed: y = r(x) r(W) forward, dx = r(d) r(W^T) backward, r = round to nearest even bf16.  Everything
else -- the xp addend, the gate math, the state update, the length mask -- is plain float64, and the state is carried
unrounded: only the operand copy of h is rounded.

Witnesses (bf16_ref.py, "Rounding flips"): a computed h or r * h within f32 error of a bf16 boundary may round either
way, so the GPU tests hand the cell the device's own operands -- hs[t] and rh[t] forward, dxp[t] backward -- and the
reference rounds THOSE after logging how far each is from its own value (max-normalised per step; the tests bound the
log by bf16_ref.WITNESS_TOL).

Bounds.  The f32 epilogue is held to gru_ref.FWD_ATOL / BWD_RTOL as the f32 forms are; the product itself to
bf16_ref.OP_TOL (|x^||W^|)_ij, the project's bound for this matrix instruction's f32 accumulation.  The product error is
carried to the outputs through the epilogue's derivatives: x 1/4 through a sigmoid, x 1 through tanh,
h_new: |du| |h - c| + |dc|, rh: |dr| |h|; backward: drh -> dr_pre x |h| r (1 - r), drh -> dh_acc x r, and the error of
dh = (dr_pre | du_pre) Wg^T + dh_acc -> dc_pre x (1 - u)(1 - c^2), du_pre x |h - c| u (1 - u) of the step before.

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import contextlib

import torch

from tests import bf16_ref as R
from tests import gru_ref as G

GRU_CFG_BF16 = 64          # csrc/gemm_tiles.h
WITNESS_TOL = R.WITNESS_TOL
OP_TOL = R.OP_TOL


class Cell:
    """step= cell of gru_ref.forward / backward with the two recurrent products routed through bf16_ref._Routed.
    rounding=False: gru_ref.cell.  wit: None, or a dict with any of
        "hs" [T+1,B,H], "rh" [T,B,H]   the device's forward operands (float32), "mask" [T,B] bool: the rows whose rh
                                       witness counts (the live form does not run finished rows);
        "dxp" [T,B,3H]                 the device's d_pre operands of the backward products.
    A product without a forward witness is witnessed by the reference's own operand rounded to float32 (what a float32
    tape holds).  logs[t] = {"h", "rh", "d_gates", "d_cand"}: distance of each witness from the reference's own value;
    scale[t] = (|h^||Wg^|, |rh^||Wc^|): the yardsticks of the two forward products."""

    def __init__(self, rounding=True, wit=None):
        self.rounding, self.wit, self.t = rounding, wit, 0
        self.logs, self.scale = [], []

    def _witness(self, t, own, key, cols, log):
        if self.wit is None:
            return None
        x = own.detach().float().to(own.dtype)
        if key in self.wit:
            w = self.wit[key][t].to(own.dtype)
            mask = self.wit.get("mask")
            x = w if mask is None or key == "hs" else torch.where(mask[t][:, None], w, x)
        d = self.wit["dxp"][t][:, cols].to(own.dtype) if "dxp" in self.wit else None
        return {"x": x, "d": d, "log": log}

    def __call__(self, xp_t, h, Wg, Wc):
        t, H = self.t, h.shape[1]
        self.t += 1
        lg, lc = {}, {}
        wg = self._witness(t, h, "hs", slice(0, 2 * H), lg)
        g = torch.sigmoid(xp_t[:, :2 * H] + R._Routed.apply(h, Wg, self.rounding, wg))
        r, u = g[:, :H], g[:, H:]
        rh = r * h
        wc = self._witness(t, rh, "rh", slice(2 * H, 3 * H), lc)
        c = torch.tanh(xp_t[:, 2 * H:] + R._Routed.apply(rh, Wc, self.rounding, wc))
        rnd = R.round_bf16 if self.rounding else (lambda x: x)
        with torch.no_grad():
            xg = (wg["x"] if wg else h).detach()
            xc = (wc["x"] if wc else rh).detach()
            self.scale.append((rnd(xg).abs() @ rnd(Wg.detach()).abs(), rnd(xc).abs() @ rnd(Wc.detach()).abs()))
        self.logs.append({"gates": lg, "cand": lc})
        return r, u, c, rh, u * h + (1 - u) * c

    def witness_distance(self):
        """the worst witness log of the run: forward operands, and the backward's once it has run"""
        return max([v for s in self.logs for d in s.values() for v in d.values()], default=0.0)


@contextlib.contextmanager
def conversion(fn):
    """bf16_ref.round_bf16 replaced by `fn` (truncate_bf16: the wrong conversion) for the duration of the block"""
    keep = R.round_bf16
    R.round_bf16 = fn
    try:
        yield
    finally:
        R.round_bf16 = keep


def forward(c, rounding=True, wit=None):
    """gru_ref.forward of a gru_ref.make_inputs case through the routed cell: (tape dict, the cell)"""
    cell = Cell(rounding, wit)
    return G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], step=cell), cell


def backward(c, outs=False, rounding=True, wit=None):
    """gru_ref.backward the same way: (dxp [T,B,3H], the cell)"""
    cell = Cell(rounding, wit)
    dxp = G.backward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], c["dh_T"], c["d_outs"] if outs else None, step=cell)
    return dxp, cell


# --------------------------------------------------------------------------------------------- bounds
def forward_bounds(ref, cell, atol=G.FWD_ATOL, op_tol=OP_TOL):
    """elementwise bound of every forward output: {name: [T,B,H]} (hs: the bound of hs[1:])"""
    T = ref["r"].shape[0]
    out = {k: [] for k in ("r", "u", "c", "rh", "hs")}
    for t in range(T):
        sg, sc = cell.scale[t]
        H = sc.shape[1]
        h, cc = ref["hs"][t], ref["c"][t]
        dr, du, dc = op_tol * sg[:, :H] / 4, op_tol * sg[:, H:] / 4, op_tol * sc
        out["r"].append(atol + dr)
        out["u"].append(atol + du)
        out["c"].append(atol + dc)
        out["rh"].append(atol + dr * h.abs())
        out["hs"].append(atol + du * (h - cc).abs() + dc)
    return {k: torch.stack(v) for k, v in out.items()}


def forward_ratio(got, ref, lens, bounds, tape_past="computed"):
    """{name: max |got - ref| / bound} over what the form writes (gru_ref.check_forward's rules for the live tape)"""
    T = ref["r"].shape[0]
    past = G.past_mask(lens.to(ref["hs"].device), T)
    worst = {}
    for name in ("hs", "r", "u", "c", "rh"):
        g, w = (got[name][1:], ref[name][1:]) if name == "hs" else (got[name], ref[name])
        ratio = (g.to(torch.float64) - w).abs() / bounds[name]
        if tape_past == "live" and name != "hs":
            ratio = torch.where(past[:, :, None], torch.zeros_like(ratio), ratio)
        worst[name] = float(ratio.nan_to_num(float("inf")).max()) if ratio.numel() else 0.0
    return worst


def check_forward(got, ref, lens, cell, tape_past="computed"):
    """gru_ref.check_forward's structural checks (written, finite, finished rows carried bit for bit, the live tape),
    then every element within its own bound.  Returns the worst |err| / bound."""
    G.check_forward(got, ref, lens, tape_past=tape_past, atol=float("inf"))
    worst = forward_ratio(got, ref, lens, forward_bounds(ref, cell), tape_past)
    if not max(worst.values()) <= 1.0:
        raise AssertionError("forward against the rounded float64 reference, worst |err| / bound: %r" % (worst,))
    return max(worst.values())


def backward_bounds(c, tape, dxp_wit, ref_dxp, rtol=G.BWD_RTOL, op_tol=OP_TOL):
    """elementwise bound of dxp [T,B,3H]: rtol x the step's own max-abs, plus the product error of the two backward GEMMs
    carried through the epilogue (module docstring).  tape: the float64 forward tape the backward ran on; dxp_wit: the
    left operands of the products (the device's dxp, or the reference's own)."""
    T, B, H3 = ref_dxp.shape
    H = H3 // 3
    rnd = R.round_bf16
    Wg, Wc = rnd(c["Wg"].to(ref_dxp.dtype)).abs(), rnd(c["Wc"].to(ref_dxp.dtype)).abs()
    d = rnd(dxp_wit.to(ref_dxp.dtype)).abs().nan_to_num(0.0)
    bound = torch.zeros_like(ref_dxp)
    for t in range(T):
        bound[t] = rtol * ref_dxp[t].abs().max()
    for t in range(T):
        h, r = tape["hs"][t].abs(), tape["r"][t].nan_to_num(0.0)
        e1 = op_tol * (d[t][:, 2 * H:] @ Wc.t())                       # drh = dc_pre Wc^T
        bound[t][:, :H] += e1 * h * r * (1 - r)
        if t == 0:
            continue
        edh = op_tol * (d[t][:, :2 * H] @ Wg.t()) + e1 * r              # dh_{t-1} = (dr_pre | du_pre) Wg^T + dh_acc
        hp, u, cc = tape["hs"][t - 1], tape["u"][t - 1].nan_to_num(0.0), tape["c"][t - 1].nan_to_num(0.0)
        bound[t - 1][:, 2 * H:] += edh * (1 - u) * (1 - cc * cc)
        bound[t - 1][:, H:2 * H] += edh * (hp - cc).abs() * u * (1 - u)
    return bound


def backward_ratio(dxp, ref_dxp, bound):
    """max |dxp - ref| / bound"""
    if not dxp.numel():
        return 0.0
    return float(((dxp.to(torch.float64) - ref_dxp).abs() / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())


def check_backward(dxp, ref_dxp, lens, bound):
    """gru_ref.check_backward's structural checks (written, finite, exactly 0 past a row's length), then every element
    within its bound.  Returns the worst |err| / bound."""
    G.check_backward(dxp, ref_dxp, lens, rtol=1e30)
    worst = backward_ratio(dxp, ref_dxp, bound)
    if not worst <= 1.0:
        raise AssertionError("backward against the rounded float64 reference: worst |err| / bound %.3f" % worst)
    return worst


# --------------------------------------------------------------------------------------------- the op test's cases
# (H, B, T): H 36 gives a k tail and ragged N = 72 / 36; B crosses a 32-, 64- and 128-row tile edge; one case at the
# models' H; and two tall cases, ragged in M, N and k, with many workgroups in both grid directions.  TALL_TILE_ROWS: the
# row threshold the GPU test hands a child process (VQA_HOT_GRU_BF16_TALL_ROWS) so that the same cases also run the
# kernel's 128 x 128 tile, which no row count selects by default: B 130 and the tall cases on the large tile, B 1 and 33
# on the small one, and the live prefix of a tall case through both.
CASES = [(H, B, T) for H in (36, 64, 128) for B in (1, 33, 130) for T in (1, 3)] + [(1024, 96, 2), (36, 2100, 2), (128, 2049, 1)]
SATURATED = (64, 33, 3)
TALL_TILE_ROWS = 100
WEIGHT_SCALE = 3.0


def make_case(H, B, T, device="cpu", sort=False):
    """gru_ref.make_inputs of a case of CASES: random lengths with 0 and T present, random h0, +-20 pre-activations in
    the SATURATED case.  The recurrent weights are three times make_inputs' scale: at its own scale the unrounded recurrence
    sits only 6 - 9 x the GPU bound from the rounded one on dxp of the T = 1, B = 1 cases (tests/test_gru_bf16_ref.py
    asks for 10 x on every case)."""
    c = G.make_inputs(T, B, H, seed=T * 7919 + B * 31 + H, device=device, saturate=(H, B, T) == SATURATED, sort=sort)
    c["Wg"], c["Wc"] = c["Wg"] * WEIGHT_SCALE, c["Wc"] * WEIGHT_SCALE
    return c
