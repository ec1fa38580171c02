"""Float64 reference of the GRU recurrence op contract (include/vqa_hot.h, section a4 / K4) and the comparator the
op-level tests judge every HIP form of the recurrence with.

Contract (time-major, r | u | c order of tf.contrib.rnn.GRUCell under tf.nn.dynamic_rnn(sequence_length)):
    xp [T,B,3H] = x_t W_x + b,  Wg_h [H,2H],  Wc_h [H,H],  len [B],  hs[0] = h0 [B,H]
    r, u = sigmoid(xp[..., :2H] + h Wg_h)             (r first)
    c    = tanh(xp[..., 2H:] + (r * h) Wc_h),  rh = r * h
    h'   = u * h + (1 - u) * c   for t < len,   h' = h   otherwise
The backward is NOT written out: dxp is torch autograd's gradient of this forward under the loss
<dh_T, h_T> + sum_t <d_outs_t, h_{t+1}>, so the kernels' own derivation of the BPTT is what the tests check.

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import torch

FWD_ATOL = 1e-5        # hs, r, u, c, rh are bounded by 1: elementwise absolute bound
BWD_RTOL = 1e-4        # dxp: per time step, relative to that step's own max-abs


def make_inputs(T, B, H, seed, lens="random", h0="random", saturate=False, device="cpu", sort=False):
    """float32 operands of one recurrence: xp [T,B,3H], Wg [H,2H], Wc [H,H], len i32 [B], h0 [B,H], dh_T [B,H] and
    d_outs [T,B,H] (zero past each row's length).
    lens     -- "random" in [0, T] with both ends present, "zero", "full", or "one_live" (one row of length T among
                rows of length 0);  sort: longest first (the live form's contract)
    h0       -- "zero" (the models start from zeros) or "random" (the API takes any initial state)
    saturate -- pre-activations of +-20 on every 5th row and every 7th column, where sigmoid / tanh and their
                derivatives reach 0 and 1 in float32"""
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, device=device, generator=g)
    ws = 0.04 * (1024.0 / H) ** 0.5              # keeps |h Wg| of the order the H = 1024 model sees
    xp = rnd(T, B, 3 * H) * 0.3
    if saturate:
        xp[:, ::5, ::7] = 20.0 * torch.sign(rnd(T, (B + 4) // 5, (3 * H + 6) // 7))
    Wg, Wc = rnd(H, 2 * H) * ws, rnd(H, H) * ws
    if lens == "random":
        ln = torch.randint(0, T + 1, (B,), device=device, generator=g, dtype=torch.int32)
        ln[0] = T
        if B > 1:
            ln[-1] = 0
    elif lens == "one_live":
        ln = torch.zeros(B, dtype=torch.int32, device=device)
        ln[B // 2] = T
    else:
        ln = torch.full((B,), T if lens == "full" else 0, dtype=torch.int32, device=device)
    if sort:
        ln = ln.sort(descending=True).values
    h = rnd(B, H) * 0.5 if h0 == "random" else torch.zeros(B, H, device=device)
    dh_T = rnd(B, H)
    d_outs = rnd(T, B, H) * 0.5 * (~past_mask(ln, T)).float()[:, :, None]
    return dict(xp=xp, Wg=Wg, Wc=Wc, lens=ln, h0=h, dh_T=dh_T, d_outs=d_outs)


def cell(xp_t, h, Wg, Wc):
    """one GRUCell step without the length mask: (r, u, c, rh, h_new)"""
    H = h.shape[1]
    g = torch.sigmoid(xp_t[:, :2 * H] + h @ Wg)
    r, u = g[:, :H], g[:, H:]
    rh = r * h
    c = torch.tanh(xp_t[:, 2 * H:] + rh @ Wc)
    return r, u, c, rh, u * h + (1 - u) * c


def forward(xp, Wg, Wc, lens, h0, dtype=torch.float64, step=cell):
    """hs [T+1,B,H] (hs[0] = h0) and the tape r, u, c, rh [T,B,H] in `dtype` on the inputs' device.  Past a row's
    length the tape holds what the cell computes from the carried state (the per-step and weight-stationary forms
    write exactly that).  `step` replaces the cell (the comparator's own tests use it to build wrong recurrences)."""
    xp, Wg, Wc, h = (t.to(dtype) for t in (xp, Wg, Wc, h0))
    lens = lens.to(device=xp.device, dtype=torch.long)
    hs, tape = [h], {k: [] for k in ("r", "u", "c", "rh")}
    for t in range(xp.shape[0]):
        r, u, c, rh, hn = step(xp[t], h, Wg, Wc)
        h = torch.where((lens > t)[:, None], hn, h)
        hs.append(h)
        for k, v in zip(("r", "u", "c", "rh"), (r, u, c, rh)):
            tape[k].append(v)
    out = {k: torch.stack(v) if v else xp.new_zeros(0, *h.shape) for k, v in tape.items()}
    out["hs"] = torch.stack(hs)
    return out


def backward(xp, Wg, Wc, lens, h0, dh_T, d_outs=None, dtype=torch.float64, step=cell):
    """dxp [T,B,3H] = (dr_pre | du_pre | dc_pre): autograd of forward() under <dh_T, h_T> + sum_t <d_outs_t, h_{t+1}>.
    d_outs [T,B,H] or None (zero past each row's length, as dynamic_rnn zeroes those outputs)."""
    with torch.enable_grad():
        x = xp.detach().to(dtype).requires_grad_(True)
        hs = forward(x, Wg, Wc, lens, h0, dtype, step)["hs"]
        loss = (dh_T.to(dtype) * hs[-1]).sum()
        if d_outs is not None:
            loss = loss + (d_outs.to(dtype) * hs[1:]).sum()
        (dxp,) = torch.autograd.grad(loss, x)
    return dxp


def past_mask(lens, T):
    """[T,B] bool: step t is past row b's length"""
    return torch.arange(T, device=lens.device)[:, None] >= lens.to(torch.long)[None, :]


def check_bits_unchanged(after, before, what, row0=None, rows=None):
    """`after` equals `before` bit for bit (NaN poison included); with row0 / rows only the batch rows outside
    [row0, row0 + rows) of axis 1 (axis 0 for a [B, ...] tensor given as 2-D) are compared."""
    a, b = after.view(torch.int32), before.view(torch.int32)
    if row0 is not None:
        axis = 1 if a.dim() == 3 else 0
        keep = torch.ones(a.shape[axis], dtype=torch.bool, device=a.device)
        keep[row0:row0 + rows] = False
        a, b = a.index_select(axis, keep.nonzero()[:, 0]), b.index_select(axis, keep.nonzero()[:, 0])
    if not torch.equal(a, b):
        raise AssertionError("%s: changed (%d words differ)" % (what, int((a != b).sum())))


def _table(rows):
    return "\n".join("  %-4s t=%-3d err %.3e  bound %.3e%s" % (n, t, e, b, "  <-- FAIL" if e > b else "")
                     for n, t, e, b in rows)


def check_forward(got, ref, lens, tape_past="computed", atol=FWD_ATOL):
    """Judge a form's forward outputs `got` (dict hs, r, u, c, rh, any float dtype) against the reference `ref`.

    tape_past -- what the form promises for the tape at t >= len:
        "computed": r, u, c, rh hold the cell's values from the carried state (per-step, weight-stationary forms);
        "live":     rh = 0 and r, u, c are not written (vqa_gru_seq_fwd_live: finished rows skip the step).
    Checks: every output (bar the unwritten live tape) fully written and finite -- hs and rh everywhere, since the
    weight-gradient GEMMs read them over all T x B rows; hs[t+1, b] bit for bit hs[len_b, b] for t >= len_b; the worst
    |err| per (tensor, step) within `atol`.  Returns {tensor: worst error}; raises AssertionError with the table."""
    T, B = ref["r"].shape[:2]
    lens = lens.to(device=ref["hs"].device, dtype=torch.long)
    past = past_mask(lens, T)
    problems, rows, worst = [], [], {}
    for name in ("hs", "r", "u", "c", "rh"):
        g, w = got[name], ref[name]
        if tuple(g.shape) != tuple(w.shape):
            raise AssertionError("%s: shape %s, want %s" % (name, tuple(g.shape), tuple(w.shape)))
        written = torch.ones(g.shape[:2], dtype=torch.bool, device=g.device)
        compared = written
        if tape_past == "live" and name != "hs":
            compared = ~past                              # rh is pinned to 0 there instead, r, u, c are not written
            if name != "rh":
                written = compared
        bad = ~torch.isfinite(g) & written[:, :, None]
        if bool(bad.any()):
            t, b, j = (int(i) for i in bad.nonzero()[0])
            problems.append("%s: %d values not written / not finite, first at t=%d row %d col %d"
                            % (name, int(bad.sum()), t, b, j))
        if tape_past == "live" and name == "rh" and bool(past.any()):
            if float(g[past].abs().max()) != 0.0:
                problems.append("rh: not zero past a row's length (live form)")
        err = (g.to(torch.float64) - w).abs()
        err = torch.where(compared[:, :, None], err, torch.zeros_like(err)).nan_to_num(float("inf"))
        per_t = err.amax(dim=(1, 2)).tolist() if err.numel() else []
        rows += [(name, t, e, atol) for t, e in enumerate(per_t)]
        worst[name] = max(per_t) if per_t else 0.0
    hs = got["hs"]
    if T and B:
        final = hs[lens, torch.arange(B, device=hs.device)]           # hs[len_b, b]
        for t in range(T):
            p = past[t]
            if bool(p.any()) and not torch.equal(hs[t + 1][p], final[p]):
                problems.append("hs[%d]: the state of a finished row is not carried bit for bit" % (t + 1))
                break
    failed = [r for r in rows if not r[2] <= r[3]]
    if failed or problems:
        raise AssertionError("forward against float64:\n" + "\n".join(problems) + "\n" + _table(failed or rows))
    return worst


def check_backward(dxp, ref_dxp, lens, rtol=BWD_RTOL):
    """Judge dxp [T,B,3H] against the reference: fully written and finite, exactly 0 for t >= len, and per time step
    max |err_t| <= rtol * max |ref_t| (a step's own scale: BPTT gradients shrink toward t = 0, and an error confined to
    a few rows, one column slab or one early step must not hide under the whole tensor's scale).  Returns the worst
    err_t / max|ref_t| over the steps; raises AssertionError with the per-step table."""
    T, B = ref_dxp.shape[:2]
    if tuple(dxp.shape) != tuple(ref_dxp.shape):
        raise AssertionError("dxp: shape %s, want %s" % (tuple(dxp.shape), tuple(ref_dxp.shape)))
    lens = lens.to(device=ref_dxp.device, dtype=torch.long)
    problems = []
    if not bool(torch.isfinite(dxp).all()):
        problems.append("dxp: %d values not written / not finite" % int((~torch.isfinite(dxp)).sum()))
    past = past_mask(lens, T)
    if bool(past.any()) and float(dxp[past].abs().nan_to_num(1.0).max()) != 0.0:
        problems.append("dxp: not exactly 0 past a row's length")
    err = (dxp.to(torch.float64) - ref_dxp).abs().nan_to_num(float("inf")).amax(dim=(1, 2)).tolist() if T else []
    scale = ref_dxp.abs().amax(dim=(1, 2)).tolist() if T else []
    rows = [("dxp", t, e, rtol * s) for t, (e, s) in enumerate(zip(err, scale))]
    failed = [r for r in rows if not r[2] <= r[3]]
    if failed or problems:
        raise AssertionError("backward against float64:\n" + "\n".join(problems) + "\n" + _table(failed or rows))
    return max([e / s for e, s in zip(err, scale) if s > 0], default=0.0)
