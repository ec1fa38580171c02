"""Float64 reference of the fused Hadamard attention + attention pooling op of include/vqa_hot.h
(vqa_attn_pool_{fwd,bwd}[_rep], csrc/attention.hip), the case matrix of its op-level tests and the comparators they
judge the kernels with.

The reference states the header's contract in plain torch, in `dtype` (float64 by default; tests/test_attn_reference.py
also evaluates it in float32, which is where the bounds below come from).  The backward is torch autograd of the
forward, never a hand-derived formula.  Every function also returns the natural scale of each output: the sum of the
magnitudes of the terms the output is a sum of, which is what a rounding error is proportional to.

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import typing

import torch

from tests.rowop_ref import Worst, check_bits, f64  # noqa: F401  (re-exported to the tests)

U = 2.0 ** -24          # unit roundoff of float32
OUTPUTS = ("att", "pooled", "dv", "dqv", "part_dw", "part_db")

# The bounds.  Every output is judged element by element:
#     |got - ref64| <= min(RT[output], (n + 2) U) * own + RTS[output] * allow
#   own    the rounding-error scale of the output with the scores given: the magnitude sum of its terms, each att[r]
#          weighted by 1 + |ln att[r]| (the argument of its exp, s - max, is rounded at its own magnitude) and each
#          datt = <dpooled, V[m, r]> taken as sqrt(sum_d (dpooled V)^2) + |datt| (the root-sum-square of the products'
#          roundings plus those of the partial sums; the magnitude sum overstates a 2048-term float32 sum 30-fold).
#          In ds = att (datt - dot) the terms datt and dot are summed, not subtracted, so the cancellation of a
#          near-one-hot row, which float32 cannot resolve, is part of the scale;
#   allow  the allowance for the score error, which every sum with att among its terms inherits whatever its own
#          summation order: the same sums with att[r] weighted by U Delta[r] = U (e[r] (1 - att[r]) + sum_{r' != r}
#          att[r'] e[r']), the first-order effect on att[r] of score errors of magnitude U e (none at nb == 1, none on
#          the top of a one-hot row).  e = sqrt(sum_h t_h^2) + |s| + |bias|, t_h = v qv w keep/keep_prob, is the
#          rounding-error scale of a float32 score (bias = 100 alone is 7.6e-6);
#   RT, RTS  each coefficient is 8x its own worst over the whole case matrix in the FLOAT32 evaluation of this
#          reference (tests/test_attn_reference.py measures them, asserts the float32 evaluation inside the bounds and
#          holds the live measurement to this table).  With ref32 the float32 evaluation and ref64s the float64
#          evaluation with ref32's score error added to its scores: RT from |ref32 - ref64s| / own, the error float32
#          adds with the scores given; RTS from |ref64s - ref64| / allow, how its score error comes through.  The
#          factor 8 covers the difference in summation order between torch's CPU reductions and a 64-lane butterfly or
#          a per-thread strided sum;
#   n      the reduction length of the output (CEIL_N): (n + 2) U is the worst-case relative forward error of an
#          n-term float32 sum with exact terms, and the coefficient of `own` never exceeds it.
#
#   output    f32 worst  RT = 8x   at                                         score: f32 worst  RTS = 8x
#   att       1.74e-07   1.4e-06   fast_fwd-rep2-R9-H256-D4096-signed-mask          3.13       25
#   pooled    3.86e-07   3.1e-06   fast_fwd-rep2-R24-H512-D4096-signed-mask         3.13       25
#   dv        5.54e-08   4.4e-07   fast_fwd-rep5-R39-H256-D2048-signed-mask         0.898      7.2
#   dqv       5.79e-08   4.6e-07   fast_fwd-rep5-R39-H256-D2048-signed-mask         1.11       8.9
#   part_dw   5.78e-08   4.6e-07   fast_bwd-rep5-R2-H1024-D1024-signed              1.11       8.9
#   part_db   2.88e-08   2.3e-07   edge-rep5-R36-H1024-D2048-bias100                0.521      4.2
#
# The ceiling (n + 2) U * (the magnitude sum; att: 2 max_r s_scale of its own value) is exceeded by the WHOLE bound in
# some cases, by the allowance and the 1 + |ln att| weights: the terms of these sums are not exact.  att carries the
# relative error 2 err(s), and the float32 evaluation itself is above (R + 2) U for pooled at R = 9 and with bias = 100.
# Largest bound / ceiling over the matrix (EXCEED; the reference tests hold every case to it) and where:
#   att       8.36     generic rep 8, R 1024, H 4: the exp and the division beside a 4-term score
#   pooled    933      rep 1, R 2, H 1024, D 2048: (R + 2) U is 4 U; w is scaled until two scores differ by 8
#   dv        30.2     the same case
#   dqv       140      rep 3, R 45, H 300, D 24 with bias = 100: (D + 2) U is 26 U, one score ulp 128 U
#   part_dw   140      the same case
#   part_db   35.1     the same case
# At the model shape (R 36, H 1024, D 2048, signed operands) the bounds are 15 to 43 times the float32 evaluation's own
# worst error for att, pooled and dv and 34 to 158 times for dqv, part_dw (a case's worst element, case by case).
#
# part_db: WIDENED against sum_r |att (datt - dot)|.  The exact gradient of the score bias is 0 for every input (a
# softmax does not see a constant added to its scores), so the reference holds float64 rounding noise and the kernel's
# value IS its rounding error.  sum_r |att (datt - dot)| cannot hold as the scale in float32: in a near-one-hot row the
# largest term rounds to exactly 0 (att = 1, dot = datt) and the error is half of that scale, in the float32
# evaluation of this reference too.  Its scales are built like every other gradient's; the magnitude sum it reports,
# sum_r att (|datt|_1 + |dot|_1), is 64 to 115 times sum_r |att (datt - dot)| at the model shape.
# Because 0 is the exact answer, a part_db that is wrong (written as 0, say) cannot show with a softmax as input:
# attn_bwd_given_att (an att that does not sum to 1, on operands without cancellation) is what pins its arithmetic.
RT = {"att": 1.4e-06, "pooled": 3.1e-06, "dv": 4.4e-07, "dqv": 4.6e-07, "part_dw": 4.6e-07, "part_db": 2.3e-07}
MEASURED_F32 = {"att": 1.74e-07, "pooled": 3.86e-07, "dv": 5.54e-08, "dqv": 5.79e-08, "part_dw": 5.78e-08,
                "part_db": 2.88e-08}
MEASURED_F32_SCORE = {"att": 3.134, "pooled": 3.134, "dv": 0.898, "dqv": 1.11, "part_dw": 1.11, "part_db": 0.521}
EXCEED = {"att": 8.36, "pooled": 933.0, "dv": 30.2, "dqv": 140.0, "part_dw": 140.0, "part_db": 35.1}
RTS = {"att": 25.0, "pooled": 25.0, "dv": 7.2, "dqv": 8.9, "part_dw": 8.9, "part_db": 4.2}
CEIL_N = {   # the reduction length of each output
    "att": lambda R, H, D, rep: H,                     # the score
    "pooled": lambda R, H, D, rep: R,
    "dv": lambda R, H, D, rep: rep * R,                # the memory's queries, each with its dot over R
    "dqv": lambda R, H, D, rep: D,                     # datt
    "part_dw": lambda R, H, D, rep: D,
    "part_db": lambda R, H, D, rep: D,
}
ROWSUM_TOL = lambda R: (R + 4) * U                    # |sum_r att - 1| of a valid row
ATT_MIN = 1e-30                                       # every case keeps its valid attention weights above this


def rt_for(name, R, H, D, rep):
    """the coefficient of the output's own scale: RT capped by the ceiling of an n-term float32 sum"""
    return min(RT[name], (CEIL_N[name](R, H, D, rep) + 2) * U)


# ---------------------------------------------------------------------------------------------------------- reference
def _mem(Q, rep, device):
    return torch.arange(Q, device=device) // rep


def _per_mem(t, rep):
    """[B*rep, ...] -> [B, rep, ...]"""
    return t.reshape((t.shape[0] // rep, rep) + tuple(t.shape[1:]))


def scores(v, qv, w, bias, keep, keep_prob, rep, dtype=torch.float64, s_delta=None):
    """s[q, r] = sum_h v[m, r, h] qv[q, h] w[h] keep[q, r, h] / keep_prob + bias, m = q // rep (before the nb mask), its
    magnitude sum sum_h |t_h| + |bias| and its rounding-error scale sqrt(sum_h t_h^2) + |s| + |bias|.
    w is [H] or one copy per query [Q, H]; bias [1] or [Q].  s_delta [Q, R]: an error added to the scores (how the bounds'
    measurement follows a float32 score error through the float64 contract)."""
    vv, q, ww, bb = f64(v, qv, w, bias, dtype=dtype)
    Q, H = q.shape
    qw = _per_mem(q * ww.reshape(-1, H), rep)                                # [B,rep,H]
    t = vv[:, None] * qw[:, :, None, :]                                      # [B,rep,R,H]: Tensor.sum, not a GEMM, so
    if keep is not None:                                                     # that float32 rounds like a plain sum
        t = t * (_per_mem(keep, rep).to(dtype) / keep_prob)
    bb = bb.reshape(-1, 1)
    s = t.sum(-1).reshape(Q, -1) + bb
    if s_delta is not None:
        s = s + s_delta.to(dtype)
    td = t.detach()
    mag = td.abs().sum(-1).reshape(Q, -1) + bb.detach().abs()
    return s, mag, (td * td).sum(-1).sqrt().reshape(Q, -1) + s.detach().abs() + bb.detach().abs()


def _attn_fwd(v, qv, V, nb, w, bias, keep, keep_prob, rep, dtype, s_delta=None):
    s, s_scale, s_err = scores(v, qv, w, bias, keep, keep_prob, rep, dtype, s_delta)
    Q, R = s.shape
    m = _mem(Q, rep, s.device)
    valid = torch.arange(R, device=s.device)[None, :] < nb.to(torch.long).to(s.device)[m][:, None]
    att = torch.softmax(s.masked_fill(~valid, float("-inf")), dim=1)
    VV = V.to(dtype)
    pooled = (_per_mem(att, rep)[:, :, :, None] * VV[:, None]).sum(2).reshape(Q, -1)
    p_scale = (_per_mem(att.detach(), rep)[:, :, :, None] * VV.abs()[:, None]).sum(2).reshape(Q, -1)     # att >= 0
    return att, pooled, s_scale, p_scale, s_err, s


def attn_fwd(v, qv, V, nb, w, bias, keep, keep_prob, rep, dtype=torch.float64):
    """v [B,R,H], qv [B*rep,H], V [B,R,D], nb [B], w [H], bias [1], keep u8 [B*rep,R,H] or None ->
    (att [B*rep,R], pooled [B*rep,D], s_scale [B*rep,R], pooled_scale [B*rep,D]).
    s[r >= nb[m]] = -inf; att = softmax_R(s) (nb <= 0: a NaN row); pooled[q] = sum_r att[q, r] V[m, r]."""
    return _attn_fwd(v, qv, V, nb, w, bias, keep, keep_prob, rep, dtype)[:4]


def _valid(nb, Q, R, rep, device):
    return torch.arange(R, device=device)[None, :] < nb.to(torch.long).to(device)[_mem(Q, rep, device)][:, None]


def _fwd_bwd(dpooled, v, qv, V, nb, w, bias, keep, keep_prob, rep, dtype, s_delta=None):
    Q, H = qv.shape
    with torch.enable_grad():
        vv, q = (t.detach().to(dtype).requires_grad_(True) for t in (v, qv))
        wq = w.detach().to(dtype).reshape(1, H).repeat(Q, 1).requires_grad_(True)
        bq = bias.detach().to(dtype).reshape(-1)[:1].repeat(Q).requires_grad_(True)
        fwd = _attn_fwd(vv, q, V, nb, wq, bq, keep, keep_prob, rep, dtype, s_delta)
        grads = torch.autograd.grad((dpooled.to(dtype) * fwd[1]).sum(), (vv, q, wq, bq))
    fwd = tuple(t.detach() for t in fwd)
    return fwd, (grads, _bwd_scales(dpooled, v, qv, V, fwd[0], w, keep, keep_prob, rep, dtype))


def attn_bwd(dpooled, v, qv, V, nb, w, bias, keep, keep_prob, rep, dtype=torch.float64):
    """autograd of <dpooled, pooled> wrt v, qv and per-query copies of w and bias:
    ((dv [B,R,H], dqv [B*rep,H], part_dw [B*rep,H], part_db [B*rep]), the four magnitude sums in the same order)"""
    return _fwd_bwd(dpooled, v, qv, V, nb, w, bias, keep, keep_prob, rep, dtype)[1]


def _bwd_scales(dpooled, v, qv, V, att, w, keep, keep_prob, rep, dtype, weight=None):
    """the magnitude sums of (dv, dqv, part_dw, part_db).  weight [B*rep,R]: the sums of an att whose element r carries
    the relative error weight[r] instead (in ds = att (datt - dot), through att itself and through dot)"""
    Q, H = qv.shape
    B, R, _ = v.shape
    dp, vv, q, VV, ww = (t.abs() for t in f64(dpooled, v, qv, V, w, dtype=dtype))
    datt = torch.einsum("bjd,brd->bjr", _per_mem(dp, rep), VV).reshape(Q, R)
    if weight is not None:
        # the rounding-error scale of a float32 datt instead of its magnitude sum: the root-sum-square of the products'
        # roundings plus the roundings of the partial sums (the magnitude sum overstates it by sqrt(D))
        sdp, sV = f64(dpooled, V, dtype=dtype)
        datt = (torch.einsum("bjd,brd->bjr", _per_mem(dp * dp, rep), VV * VV).sqrt()
                + torch.einsum("bjd,brd->bjr", _per_mem(sdp, rep), sV).abs()).reshape(Q, R)
    dot = (att * datt).sum(1, keepdim=True)
    if weight is None:
        ds = att * (datt + dot)
    else:
        ds = att * (weight * (datt + dot) + (att * weight * datt).sum(1, keepdim=True))
    ds = _per_mem(ds, rep)                                                  # [B,rep,R]
    qw = _per_mem(q * ww, rep)                                              # [B,rep,H]
    if keep is None:
        sv = torch.einsum("bjr,brh->bjh", ds, vv)
        dv = torch.einsum("bjr,bjh->brh", ds, qw)
    else:
        k = _per_mem(keep, rep).to(dtype) / keep_prob                       # [B,rep,R,H]
        sv = torch.einsum("bjr,bjrh,brh->bjh", ds, k, vv)
        dv = torch.einsum("bjr,bjrh,bjh->brh", ds, k, qw)
    sv = sv.reshape(Q, H)
    return dv, sv * ww, sv * q, ds.reshape(Q, R).sum(1)


def attn_bwd_given_att(dpooled, V, att, rep, dtype=torch.float64):
    """part_db of the backward as the function of its `att` INPUT that the header states (ds = att (datt - sum_r att
    datt), datt = <dpooled, V[m, r]>, part_db = sum_r ds), for an att that is no softmax: it is then
    dot (1 - sum_r att), not 0.  Returns (part_db [B*rep], its magnitude sum)."""
    dp, VV, a = f64(dpooled, V, att, dtype=dtype)
    Q, R = a.shape
    datt = torch.einsum("bjd,brd->bjr", _per_mem(dp, rep), VV).reshape(Q, R)
    ds = a * (datt - (a * datt).sum(1, keepdim=True))
    mag = torch.einsum("bjd,brd->bjr", _per_mem(dp.abs(), rep), VV.abs()).reshape(Q, R)
    return ds.sum(1), (a.abs() * (mag + (a.abs() * mag).sum(1, keepdim=True))).sum(1)


# ------------------------------------------------------------------------------------------------------------- cases
class Case(typing.NamedTuple):
    family: str
    rep: int
    R: int
    H: int
    D: int
    kind: str = "signed"
    mask: bool = False
    fasts: tuple = (1,)          # the vqa_attn_set_fast settings the GPU test runs it under
    B: int = 4
    nb: tuple = None             # None: nb_cycle

    def id(c):
        return "%s-rep%d-R%d-H%d-D%d-%s%s" % (c.family, c.rep, c.R, c.H, c.D, c.kind, "-mask" if c.mask else "")


# The form table of the fast forward (csrc/attention.hip: FwdFast, FwdRep, FwdRepD1024), by dispatch route: the rows of V
# a thread prefetches (PF) and the rows per pooling batch.  Every form scores rows in batches of 8 (one per wave).
FWD_FORMS = {"fwd_fast": dict(PF=8, BATCH=7), "fwd_rep": dict(PF=4, BATCH=6), "fwd_rep_d1024": dict(PF=6, BATCH=6)}


def form_R(routes, kept):
    """The R values of the fast forward cases that run on `routes`: `kept` (the values the matrix always had, in their
    order: a case's keep mask goes by its position) and then, for every route, whichever of these is missing: 1, the
    prefetch edge PF-1, PF, PF+1, the first pooling batch's end PF+BATCH and PF+BATCH+1, the score-row batch edges 8/9,
    16/17, 24/25, 32/33, and 36, 39, 40.
    The added values follow in descending order.  Either order covers both masks on both sides of every edge; in ascending
    order one added case (fast_fwd-rep2-R5-H512-D2048-signed-mask) has a float32 evaluation of part_db, whose exact value
    is 0, of 5.12e-08 of its scale, 1.78x the table's worst, and the table would no longer be the live measurement."""
    want = {1, 8, 9, 16, 17, 24, 25, 32, 33, 36, 39, 40}
    for f in (FWD_FORMS[r] for r in routes):
        want |= {f["PF"] - 1, f["PF"], f["PF"] + 1, f["PF"] + f["BATCH"], f["PF"] + f["BATCH"] + 1}
    return list(kept) + sorted((R for R in want - set(kept) if R >= 1), reverse=True)


FAST_R = form_R(("fwd_fast", "fwd_rep"), kept=(1, 2, 7, 8, 9, 14, 15, 16, 23, 24, 25, 32, 33, 36, 39, 40))
D1024_R = form_R(("fwd_rep_d1024",), kept=(1, 4, 5, 10, 11, 17, 36, 40))
FAST_BWD_R = [1, 2, 7, 8, 9, 15, 16, 17, 24, 33, 36, 39, 40]
KINDS = ["signed", "bias100", "peak", "equal", "zero_keep", "ones_mask", "dp_zero"]


def fast_fwd_cases(H, D):
    """attn_pool_fwd_form_kernel<FwdFast, H/256, D, MASK> (rep 1 under 1, rep 2 under 2 and 3, rep 5 under 3) and
    attn_pool_fwd_form_kernel<FwdRep, H/256, D, MASK> (rep 5 under 1 and 2), each beside the generic kernel (0, and rep 2
    under 1); the mask alternates along FAST_R, so each MASK instance takes half of the R values"""
    out = []
    for i, R in enumerate(FAST_R):
        mask = (i + H // 256 + D // 2048) % 2 == 0
        out.append(Case("fast_fwd", 1, R, H, D, mask=mask, fasts=(0, 1)))
        both = (H, D) == (1024, 2048)          # the model shape also runs 2: rep 2 then leaves the generic kernel
        out.append(Case("fast_fwd", 5, R, H, D, mask=mask, fasts=(0, 1, 2, 3) if both else (0, 1, 3)))
        out.append(Case("fast_fwd", 2, R, H, D, mask=not mask, fasts=(0, 1, 2, 3) if both else (0, 3)))
    return out


def d1024_cases():
    """attn_pool_fwd_form_kernel<FwdRepD1024, 4, 1024, MASK> + attn_pool_bwd_fast_kernel<5, MASK, 1024> (rep 5 under 1 and 2; under
    3 the forward is the generic kernel); rep 1 is generic under every setting"""
    out = []
    for i, R in enumerate(D1024_R):
        out.append(Case("d1024", 5, R, 1024, 1024, mask=i % 2 == 0, fasts=(0, 1, 2, 3)))
        out.append(Case("d1024", 1, R, 1024, 1024, mask=i % 2 == 1, fasts=(0, 1)))
    return out


def generic_cases():
    """attn_pool_fwd_kernel and attn_pool_bwd_kernel<1 | 5 | 8> at shapes every fast form refuses"""
    G = lambda rep, R, H, D, mask: Case("generic", rep, R, H, D, mask=mask)
    return [
        G(1, 41, 4, 4, False),            # bwd<1>; the smallest H and D
        G(2, 63, 12, 24, True),           # bwd<5> with rep < REP; R one below the softmax's 64-lane stride
        G(3, 64, 300, 1024, True),        # bwd<5>; R on the stride; H4 = 75 leaves threads without a column
        G(4, 65, 1028, 2052, False),      # bwd<5>; R one above the stride; H > 1024: the second hu0 pass; D % 2048 != 0
        G(5, 100, 2048, 24, True),        # bwd<5> with rep == REP; two full hu0 passes
        G(6, 129, 300, 4, False),         # bwd<8> with rep < REP; R = 2 * 64 + 1
        G(7, 41, 12, 6144, True),         # bwd<8>; the largest D
        G(8, 1024, 4, 24, True),          # bwd<8> with rep == REP; R = MAX_R
        G(1, 1024, 12, 4, False),         # bwd<1>; R = MAX_R
        G(8, 64, 1028, 1024, True),       # bwd<8>; the second hu0 pass with 8 queries
        G(1, 65, 2048, 6144, False),      # bwd<1>; the largest H and D together
        G(1, 41, 1024, 2048, False),      # a model shape but R = 41: both fast forms refuse
        G(5, 41, 1024, 2048, True),       # the same at rep 5
        G(5, 36, 1024, 2052, True),       # D % 2048 != 0
        G(1, 36, 1280, 2048, True),       # H % 256 == 0 but H > 1024
        G(2, 36, 1024, 2048, True),       # rep 2 under 1: generic forward, bwd<5> at the model shape
        G(4, 36, 256, 2048, False),       # rep 4 under 1
        G(8, 36, 1024, 2048, True),       # rep 8: bwd<8> at the model shape
        G(6, 9, 512, 4096, True),         # rep 6
    ]


def fast_bwd_cases():
    """attn_pool_bwd_fast_kernel<1 | 5, MASK> (D 2048) and <5, MASK, 1024> under 1 beside the generic backward (0);
    rep 1 at D 1024 is the generic backward under every setting"""
    out = []
    for D in (2048, 1024):
        for i, R in enumerate(FAST_BWD_R):
            mask = (i + D // 1024) % 2 == 0
            out.append(Case("fast_bwd", 1, R, 1024, D, mask=mask, fasts=(0, 1)))
            out.append(Case("fast_bwd", 5, R, 1024, D, mask=not mask, fasts=(0, 1)))
    return out


EDGE_SHAPES = [            # (rep, R, H, D, fasts)
    (1, 36, 1024, 2048, (0, 1)),        # fwd_fast<4, 2048> + bwd_fast<1>: the VQA models' step
    (5, 36, 1024, 2048, (0, 1, 3)),     # fwd_rep<4, 2048> / fwd_fast<4, 2048> + bwd_fast<5>: the pre-training step
    (3, 45, 300, 24, (1,)),             # generic forward, bwd<5>
]


def edge_cases():
    """every data edge at two fast shapes and one generic shape, with and without the keep mask"""
    out = []
    for rep, R, H, D, fasts in EDGE_SHAPES:
        for kind in KINDS:
            for mask in (False, True):
                if kind in ("zero_keep", "ones_mask") and not mask:
                    continue
                if kind == "dp_zero" and rep == 1:
                    continue
                out.append(Case("edge", rep, R, H, D, kind=kind, mask=mask, fasts=fasts))
    return out


def nb0_cases():
    """nb == 0 in the middle memory of three"""
    N = lambda rep, R, H, D, fasts, mask: Case("nb0", rep, R, H, D, mask=mask, fasts=fasts, B=3, nb=(R, 0, 2))
    return [N(1, 36, 1024, 2048, (0, 1), True),         # fwd_fast + bwd_fast<1>
            N(5, 36, 1024, 2048, (0, 1, 3), True),      # fwd_rep<4, 2048> (five queries share the workgroup's LDS)
            N(5, 36, 1024, 1024, (0, 1), False),        # fwd_rep_d1024 + bwd_fast<5, ., 1024>
            N(3, 45, 300, 24, (1,), True)]              # generic


def matrix():
    out = []
    for H in (256, 512, 768, 1024):
        for D in (2048, 4096):
            out += fast_fwd_cases(H, D)
    return out + d1024_cases() + generic_cases() + fast_bwd_cases() + edge_cases() + nb0_cases()


def nb_cycle(B, R):
    """nb in {1, 2, R-1, R} (clamped into [1, R]), one value per memory in turn"""
    return torch.tensor([min(max(x, 1), R) for x in ([1, 2, R - 1, R] * B)[:B]], dtype=torch.int32)


def make_case(c, seed=0):
    """the inputs of Case c as float32 / int32 / uint8 CPU tensors (a dict), seeded by the case itself"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * c.R + 31 * c.H + 17 * c.D + 3 * c.rep + KINDS.index(c.kind)
                                      + (500 if c.mask else 0))
    B, rep, R, H, D = c.B, c.rep, c.R, c.H, c.D
    Q = B * rep
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    v, qv, V, w, dp = rn(B, R, H), rn(Q, H), rn(B, R, D), rn(H), rn(Q, D)
    bias = torch.tensor([0.2], dtype=torch.float64)
    nb = torch.tensor(c.nb, dtype=torch.int32) if c.nb is not None else nb_cycle(B, R)
    keep_prob, keep = 0.8, None
    if c.mask:
        keep = (torch.rand(Q, R, H, generator=g) < 0.8).to(torch.uint8)
    if c.kind == "ones_mask":
        keep, keep_prob = torch.ones(Q, R, H, dtype=torch.uint8), 1.0
    if c.kind == "zero_keep":
        keep[1] = 0                       # query 1's score is the bias alone: uniform attention over nb
    if c.kind == "equal":
        v = torch.zeros_like(v)
    if c.kind == "bias100":
        bias = torch.tensor([100.0], dtype=torch.float64)
    if c.kind == "peak":
        qv = qv.abs()
    if c.kind == "dp_zero":
        dp[2] = 0.0                       # the third query of memory 0
    valid = (torch.arange(R)[None, :] < nb.long()[_mem(Q, rep, None)][:, None])

    def spread():
        s = scores(v, qv, w, bias, keep, keep_prob, rep)[0]
        hi = s.masked_fill(~valid, float("-inf")).amax(1)
        lo = s.masked_fill(~valid, float("inf")).amin(1)
        d = (hi - lo)[valid.any(1)]
        return s, float(d.max()) if d.numel() else 0.0
    # w is scaled so that the widest range of one query's valid scores is 8 (60 with bias = 100: about +-30)
    _, rng = spread()
    if rng > 0:
        w = w * ((60.0 if c.kind == "bias100" else 8.0) / rng)
    if c.kind == "peak":
        # the last valid region of every memory scores >= 40 above the rest for every query of the memory
        s, _ = spread()
        k = keep.double() / keep_prob if keep is not None else torch.ones(Q, R, H, dtype=torch.float64)
        for mem in range(B):
            n = int(nb[mem])
            if n < 2:
                continue
            t = 0.0
            for q in range(mem * rep, (mem + 1) * rep):
                gain = float((qv[q] * w.abs() * k[q, n - 1]).sum())
                if gain > 0:
                    t = max(t, (40.0 + float(s[q, :n].max() - s[q, n - 1])) / gain)
            v[mem, n - 1] += t * torch.sign(w)
    case = dict(v=v.float(), qv=qv.float(), V=V.float(), nb=nb, w=w.float(), bias=bias.float(), keep=keep,
                keep_prob=keep_prob, rep=rep, dpooled=dp.float())
    # the smallest valid attention weight stays far above the float32 denormal range
    sc = scores(case["v"], case["qv"], case["w"], case["bias"], keep, keep_prob, rep)[0]
    att = torch.softmax(sc.masked_fill(~valid, float("-inf")), dim=1)
    ok = valid & ~torch.isnan(att)
    if bool(ok.any()):
        assert float(att[ok].min()) > ATT_MIN, "%s: smallest valid attention weight %.3e" % (c.id(), float(att[ok].min()))
    return case


def fwd_args(case, dtype=torch.float64):
    return (case["v"], case["qv"], case["V"], case["nb"], case["w"], case["bias"], case["keep"], case["keep_prob"],
            case["rep"], dtype)


def reference(case, dtype=torch.float64, s_delta=None):
    """(att, pooled, s_scale, pooled_scale, s_err, s), ((dv, dqv, part_dw, part_db), their magnitude sums) of a case"""
    return _fwd_bwd(case["dpooled"], *fwd_args(case, dtype), s_delta=s_delta)


# --------------------------------------------------------------------------------------------------------- comparators
def _lead(t, like):
    """[leading axis] -> broadcastable over `like`"""
    return t.reshape([-1] + [1] * (like.dim() - 1))


def bounds(ref, case, dims):
    """{output: (reference, own scale, allowance scale, bound, ceiling)} of the float64 reference `ref`, elementwise:
    bound = rt_for(output) * own scale + RTS[output] * allowance scale"""
    ref_fwd, (grads, gscales) = ref
    att, pooled, s_scale, p_scale, e = (t.detach().to(torch.float64) for t in ref_fwd[:5])
    rep, nb, dev = case["rep"], case["nb"], att.device
    Q, R = att.shape
    valid = _valid(nb, Q, R, rep, dev)
    a = att.masked_fill(~valid, 0.0)
    # exp's argument s - max is rounded at its own magnitude: att[r] carries the relative error U (1 + |ln att[r]|)
    L = 1.0 - torch.log(a.clamp_min(1e-300)).masked_fill(a == 0, 0.0)
    # a score error of magnitude U e reaches att[r] as the relative error U Delta[r] = U (e[r] (1 - att[r]) + sum_{r' != r}
    # att[r'] e[r']): none at nb == 1, none on the top of a one-hot row
    ae = a * e.masked_fill(~valid, 0.0)
    Delta = U * (e.masked_fill(~valid, 0.0) * (1.0 - a) + (ae.sum(1, keepdim=True) - ae))
    absV = case["V"].to(dev).to(torch.float64).abs()
    pool = lambda wgt: torch.einsum("bjr,brd->bjd", _per_mem(a * wgt, rep), absV).reshape(Q, -1)
    args = (case["dpooled"], case["v"], case["qv"], case["V"], a, case["w"], case["keep"], case["keep_prob"], rep,
            torch.float64)
    own = {"att": a * L, "pooled": pool(L)}
    allow = {"att": a * Delta, "pooled": pool(Delta)}
    own.update(zip(OUTPUTS[2:], _bwd_scales(*args, weight=L)))
    allow.update(zip(OUTPUTS[2:], _bwd_scales(*args, weight=Delta)))
    refs = dict(zip(OUTPUTS, (att, pooled) + tuple(grads)))
    scales = dict(zip(OUTPUTS, (att, p_scale) + tuple(gscales)))
    smax = s_scale.masked_fill(~valid, 0.0).amax(1)
    out = {}
    for name in OUTPUTS:
        r = refs[name].detach().to(torch.float64)
        o, al, sc = (t.detach().to(torch.float64).to(dev).expand_as(r) for t in (own[name], allow[name], scales[name]))
        bound = rt_for(name, *dims) * o + RTS[name] * al
        ceil = sc * (CEIL_N[name](*dims) + 2) * U * (_lead(2.0 * smax, r) if name == "att" else 1.0)
        out[name] = (r, o, al, bound, ceil)
    return out


def within(got, ref, bound, what=""):
    """The worst |got - ref| / bound over the elements (0 where the error is 0; an error on a zero bound is infinite).
    Where the reference is NaN (an nb == 0 memory) `got` must be NaN, everywhere else finite.  Raises AssertionError
    naming the worst element if any error exceeds its bound."""
    if tuple(got.shape) != tuple(ref.shape):
        raise AssertionError("%s: shape %s, want %s" % (what, tuple(got.shape), tuple(ref.shape)))
    g = got.detach().to(torch.float64)
    r = ref.detach().to(torch.float64).to(g.device)
    nan = torch.isnan(r)
    wrong = (torch.isnan(g) != nan) | (torch.isinf(g) & ~nan)
    if bool(wrong.any()):
        first = tuple(int(i) for i in wrong.nonzero()[0])
        raise AssertionError("%s: %d values NaN / infinite where the reference is not (or the reverse), first at %s"
                             % (what, int(wrong.sum()), first))
    if g.numel() == 0:
        return 0.0
    err = (g - r).abs().masked_fill(nan, 0.0)
    bound = bound.to(torch.float64).to(g.device).expand_as(r).masked_fill(nan, 1.0)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max())
    if worst > 1.0:
        at = tuple(int(i) for i in torch.unravel_index(ratio.reshape(-1).argmax(), ratio.shape)) if ratio.dim() else ()
        raise AssertionError("%s: %d of %d elements out of bounds, worst at %s: got %.9g want %.9g, err %.3e bound %.3e"
                             % (what, int((ratio > 1).sum()), g.numel(), at, float(g[at]), float(r[at]),
                                float(err[at]), float(bound[at])))
    return worst


def compare(names, got, ref, case, dims, worst=None, tag=""):
    """the outputs `names` against the float64 reference; returns {output: worst fraction of its bound}"""
    b = bounds(ref, case, dims)
    out = {}
    for name, g in zip(names, got):
        out[name] = within(g, b[name][0], b[name][3], "%s %s" % (tag, name))
        if worst is not None:
            worst.add(("%s %s" % (tag.split(" ")[0], name)).strip(), out[name])
    return out


def compare_fwd(got_att, got_pooled, ref, case, dims, worst=None, tag=""):
    return compare(OUTPUTS[:2], (got_att, got_pooled), ref, case, dims, worst, tag)


def compare_bwd(got, ref, case, dims, worst=None, tag=""):
    return compare(OUTPUTS[2:], got, ref, case, dims, worst, tag)


def measure(case, dims):
    """What the coefficients are measured from, for one case.  ref32 = the float32 evaluation, ref64s = the float64
    evaluation with the float32 evaluation's score error added to its scores:
    {output: max |ref32 - ref64s| / own scale}                 the error float32 adds with the scores given (-> RT),
    {"score " + output: max |ref64s - ref64| / allowance scale}  how its score error comes through (-> RTS),
    {"exceed " + output: max bound / ceiling}.  Returns (that dict, ref64, ref32)."""
    ref64, ref32 = reference(case), reference(case, torch.float32)
    ds = (ref32[0][5].to(torch.float64) - ref64[0][5])
    ds = ds.masked_fill(~_valid(case["nb"], ds.shape[0], ds.shape[1], case["rep"], ds.device), 0.0)
    ref64s = reference(case, s_delta=ds)
    flat = lambda ref: dict(zip(OUTPUTS, tuple(ref[0][:2]) + tuple(ref[1][0])))
    x32, x64s = flat(ref32), flat(ref64s)
    out = {}
    for name, (r, own, allow, bound, ceil) in bounds(ref64, case, dims).items():
        fin = ~torch.isnan(r)
        for key, num, den in ((name, (x32[name].to(torch.float64) - x64s[name]).abs(), own),
                              ("score " + name, (x64s[name] - r).abs(), allow), ("exceed " + name, bound, ceil)):
            ok = fin & (den > 0)
            if bool(ok.any()):
                out[key] = float((num / den)[ok].max())
    return out, ref64, ref32
