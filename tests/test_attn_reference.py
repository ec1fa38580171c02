"""The float64 attention reference (tests/attn_ref.py) that tests/test_gpu_attn_f64.py judges the kernels against: it
reproduces the oracle's independent forward, its autograd backward agrees with central finite differences, it gives the
closed-form answers, its comparators reject the mistakes a kernel could make, and its FLOAT32 evaluation stays inside
the bounds on every case of the GPU matrix.  That evaluation is where the bounds come from: each coefficient of
attn_ref.RT / RTS is 8x the worst the module measures (and prints), the tables in attn_ref.py are held to the live
measurement, and the whole bound of every case is held to the stated multiple of its float32 sum ceiling."""
import numpy as np
import pytest
import torch

from oracle import vqa_oracle as O
from tests import attn_ref as A

def _dims(c):
    return (c.R, c.H, c.D, c.rep)


def _groups():
    out = {}
    for c in A.matrix():
        key = c.family if c.family != "fast_fwd" else "fast_fwd-H%d-D%d" % (c.H, c.D)
        out.setdefault(key, []).append(c)
    return out


GROUPS = _groups()


@pytest.fixture(scope="module")
def evaluated():
    """The float32 evaluation of the reference against its float64 evaluation on every case of the GPU matrix, once:
    ({group: [failures at the bounds]}, {coefficient: (worst, case)}) -- what attn_ref.RT and EXCEED are set from."""
    failures, worst = {}, {}
    for group, cases in GROUPS.items():
        failures[group] = []
        for c in cases:
            case = A.make_case(c)
            m, ref64, ref32 = A.measure(case, _dims(c))
            try:
                A.compare_fwd(ref32[0][0], ref32[0][1], ref64, case, _dims(c), tag=c.id())
                A.compare_bwd(ref32[1][0], ref64, case, _dims(c), tag=c.id())
            except AssertionError as e:
                failures[group].append(str(e))
            for k, x in m.items():
                if x > worst.get(k, (-1.0, None))[0]:
                    worst[k] = (x, c.id())
    print("\nfloat32 evaluation of attn_ref against float64, worst per coefficient and where:\n"
          + "\n".join("  %-16s %.3e  %s" % (k, x, where) for k, (x, where) in sorted(worst.items())))
    return failures, worst


# --------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("drop", [False, True])
def test_forward_matches_the_oracle_at_rep_1(drop):
    rng = np.random.default_rng(3)
    B, R, H, D = 5, 9, 12, 8
    v, qv, V = rng.standard_normal((B, R, H)), rng.standard_normal((B, H)), rng.standard_normal((B, R, D))
    w, bias = rng.standard_normal((H, 1)) * 0.3, np.array([0.2])
    nb = np.array([1, 2, R - 1, R, 5], np.int32)
    keep = (rng.random((B, R, H)) < O.KEEP_ATT).astype(np.float64)
    # without dropout the oracle takes mask = keep_prob, so that mask / keep_prob == 1
    att_o, _ = O.hadamard_attention_forward(v, nb, qv, w, bias, keep if drop else np.full_like(keep, O.KEEP_ATT))
    pooled_o = np.einsum("br,brd->bd", att_o, V)
    t = torch.from_numpy
    att, pooled, s_scale, p_scale = A.attn_fwd(t(v), t(qv), t(V), t(nb), t(w[:, 0]), t(bias),
                                               t(keep.astype(np.uint8)) if drop else None, O.KEEP_ATT, 1)
    np.testing.assert_allclose(att.numpy(), att_o, rtol=1e-13, atol=0)
    np.testing.assert_allclose(pooled.numpy(), pooled_o, rtol=0, atol=1e-14)
    m = keep / O.KEEP_ATT if drop else 1.0
    np.testing.assert_allclose(s_scale.numpy(), np.abs(v * qv[:, None, :] * w[None, None, :, 0] * m).sum(-1) + 0.2,
                               rtol=1e-13)
    np.testing.assert_allclose(p_scale.numpy(), np.einsum("br,brd->bd", att_o, np.abs(V)), rtol=1e-13)


# ------------------------------------------------------------------------------------------------- finite differences
@pytest.mark.parametrize("rep,mask", [(1, False), (3, True)])
def test_backward_matches_central_finite_differences(rep, mask):
    c = A.Case("fd", rep, 5, 4, 3, mask=mask, B=2, nb=(5, 3))
    case = {k: (x.double() if torch.is_tensor(x) and x.is_floating_point() else x) for k, x in A.make_case(c).items()}
    Q, H = case["qv"].shape
    (dv, dqv, pdw, pdb), _ = A.attn_bwd(case["dpooled"], *A.fwd_args(case))

    def loss(v, qv, w, bias):
        return float((case["dpooled"] * A.attn_fwd(v, qv, case["V"], case["nb"], w, bias, case["keep"],
                                                   case["keep_prob"], rep)[1]).sum())
    base = [case["v"], case["qv"], case["w"].reshape(1, H).repeat(Q, 1), case["bias"].repeat(Q)]
    eps = 1e-6
    for which, grad in ((0, dv), (1, dqv), (2, pdw), (3, pdb)):
        grad = grad.contiguous()
        fd = torch.zeros_like(grad)
        for i in range(grad.numel()):
            hi, lo = [x.clone() for x in base], [x.clone() for x in base]
            hi[which].view(-1)[i] += eps
            lo[which].view(-1)[i] -= eps
            fd.view(-1)[i] = (loss(*hi) - loss(*lo)) / (2 * eps)
        assert float((fd - grad).abs().max()) <= 1e-8 * max(1.0, float(grad.abs().max())), which
    assert float(pdb.abs().max()) < 1e-15          # a softmax does not see a constant added to its scores


# ------------------------------------------------------------------------------------------------------ known answers
def test_closed_form_answers():
    g = torch.Generator().manual_seed(5)
    B, rep, R, H, D = 4, 2, 7, 8, 6
    Q = B * rep
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    v, qv, V, w, bias = rn(B, R, H), rn(Q, H), rn(B, R, D), rn(H), torch.tensor([0.3], dtype=torch.float64)
    nb = torch.tensor([1, 2, R - 1, R], dtype=torch.int32)
    m = torch.arange(Q) // rep
    valid = torch.arange(R)[None, :] < nb.long()[m][:, None]
    uniform = valid.double() / nb.double()[m][:, None]

    # equal scores (v == 0): att == 1 / nb over the valid regions, 0 elsewhere
    att, pooled, _, _ = A.attn_fwd(torch.zeros_like(v), qv, V, nb, w, bias, None, 1.0, rep)
    assert torch.allclose(att, uniform, rtol=1e-15, atol=0)
    assert torch.allclose(pooled, torch.einsum("qr,qrd->qd", uniform, V[m]), rtol=0, atol=1e-15)
    # nb == 1: a one-hot row and pooled == V[:, 0]
    att, pooled, _, _ = A.attn_fwd(v, qv, V, nb, w, bias, None, 1.0, rep)
    assert torch.equal(att[:rep], torch.eye(R, dtype=torch.float64)[:1].repeat(rep, 1))
    assert torch.equal(pooled[:rep], V[0, 0][None, :].repeat(rep, 1))
    assert bool((att[~valid] == 0).all())
    # an all-zero keep mask: the score is the bias alone, so the attention is uniform over nb
    att0, _, s_scale, _ = A.attn_fwd(v, qv, V, nb, w, bias, torch.zeros(Q, R, H, dtype=torch.uint8), 0.8, rep)
    assert torch.allclose(att0, uniform, rtol=1e-15, atol=0)
    assert torch.equal(s_scale, torch.full_like(s_scale, 0.3))
    # a constant added to the bias changes nothing
    att_b, pooled_b, _, _ = A.attn_fwd(v, qv, V, nb, w, bias + 7.0, None, 1.0, rep)
    assert torch.allclose(att_b, att, rtol=1e-13, atol=0) and torch.allclose(pooled_b, pooled, rtol=0, atol=1e-13)
    # memory m = q // rep: query 3 attends over memory 1
    att1, pooled1, _, _ = A.attn_fwd(v[1:2], qv[3:4], V[1:2], nb[1:2], w, bias, None, 1.0, 1)
    assert torch.equal(att1[0], att[3]) and torch.equal(pooled1[0], pooled[3])
    # nb <= 0: a NaN row, and only that memory's
    attn, pooledn, _, _ = A.attn_fwd(v, qv, V, torch.tensor([R, 0, -1, 2], dtype=torch.int32), w, bias, None, 1.0, rep)
    assert bool(torch.isnan(attn[rep:3 * rep]).all()) and bool(torch.isnan(pooledn[rep:3 * rep]).all())
    assert not bool(torch.isnan(attn[:rep]).any()) and not bool(torch.isnan(pooledn[3 * rep:]).any())


def test_given_att_backward_is_the_autograd_backward_for_a_softmax_and_dot_times_deficit_otherwise():
    c = A.Case("t", 2, 6, 8, 12, mask=True, B=2, nb=(6, 4))
    case = A.make_case(c)
    ref_fwd, ((_, _, _, pdb), _) = A.reference(case)
    got, mag = A.attn_bwd_given_att(case["dpooled"], case["V"], ref_fwd[0], 2)
    assert float((got - pdb).abs().max()) <= 1e-15 * float(mag.max())
    half, _ = A.attn_bwd_given_att(case["dpooled"], case["V"], 0.5 * ref_fwd[0], 2)
    m = torch.arange(4) // 2
    dot = torch.einsum("qr,qd,qrd->q", ref_fwd[0], case["dpooled"].double(), case["V"].double()[m])
    assert torch.allclose(half, 0.25 * dot, rtol=1e-12, atol=0)        # c (1 - c) dot at c = 1/2


# -------------------------------------------------------------------------------------------------------- comparators
def _f32_outputs(case):
    fwd, (grads, _) = A.reference(case, torch.float32)
    return fwd[0], fwd[1], list(grads)


def test_comparators_reject_what_a_kernel_could_get_wrong():
    c = A.Case("edge", 5, 36, 256, 2048, mask=True, B=4)
    case = A.make_case(c)
    ref = A.reference(case)
    ref_fwd, ref_bwd = ref
    att, pooled, grads = _f32_outputs(case)
    A.compare_fwd(att, pooled, ref, case, _dims(c))
    A.compare_bwd(grads, ref, case, _dims(c))
    m = torch.arange(20) // 5
    last = (case["nb"].long()[m] - 1)
    # the pooling weight of the last valid region halved for one query
    bad = pooled.clone()
    bad[7] -= 0.5 * att[7, last[7]] * case["V"][m[7], last[7]]
    with pytest.raises(AssertionError, match="pooled"):
        A.compare_fwd(att, bad, ref, case, _dims(c))
    # one attention weight off by 1e-4 of itself
    bad = att.clone()
    bad[11, 0] *= 1 + 1e-4
    with pytest.raises(AssertionError, match="att"):
        A.compare_fwd(bad, pooled, ref, case, _dims(c))
    # a masked region that is not exactly 0
    bad = att.clone()
    bad[0, 35] = 1e-30
    with pytest.raises(AssertionError, match="att"):
        A.compare_fwd(bad, pooled, ref, case, _dims(c))
    # 1 / keep_prob missing from the backward's mask multiply: dv is 0.8 of itself
    with pytest.raises(AssertionError, match="dv"):
        A.compare_bwd([grads[0] * case["keep_prob"]] + grads[1:], ref, case, _dims(c))
    # one query's dqv taken from its neighbour; one element of part_dw unwritten
    bad = grads[1].clone()
    bad[6] = bad[5]
    with pytest.raises(AssertionError, match="dqv"):
        A.compare_bwd([grads[0], bad] + grads[2:], ref, case, _dims(c))
    bad = grads[2].clone()
    bad[19, 255] = float("nan")
    with pytest.raises(AssertionError, match="part_dw"):
        A.compare_bwd(grads[:2] + [bad, grads[3]], ref, case, _dims(c))
    # a score-bias gradient of the size of one ds term
    bad = grads[3].clone()
    bad[3] += 1e-3 * float(ref_bwd[1][3][3])
    with pytest.raises(AssertionError, match="part_db"):
        A.compare_bwd(grads[:3] + [bad], ref, case, _dims(c))


# ------------------------------------------------------------------------- the float32 evaluation over the GPU matrix
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_float32_evaluation_is_inside_the_bounds(group, evaluated):
    assert not evaluated[0][group], "\n".join(evaluated[0][group])


def test_the_table_is_the_live_measurement_and_every_bound_is_held_to_its_ceiling(evaluated):
    _, worst = evaluated
    for table, rts, prefix in ((A.MEASURED_F32, A.RT, ""), (A.MEASURED_F32_SCORE, A.RTS, "score ")):
        for name in A.OUTPUTS:
            live, where = worst[prefix + name]
            # the table is what this run measures (torch's reduction order may move it a little); RT, RTS are 8x it
            assert 0.8 * table[name] <= live <= 1.05 * table[name], (prefix + name, live, where)
            assert 7.6 * table[name] <= rts[name] <= 8.4 * table[name], prefix + name
    for name in A.OUTPUTS:
        # the whole bound (score allowance included) against (n + 2) U scale, per case: no further than the table says
        live = worst["exceed " + name][0]
        assert live <= A.EXCEED[name] <= 1.1 * live, (name, live, worst["exceed " + name][1])
    for c in A.matrix():
        for name in A.OUTPUTS:
            assert A.rt_for(name, *_dims(c)) <= min(A.RT[name], (A.CEIL_N[name](*_dims(c)) + 2) * A.U)


def test_the_matrix_reaches_every_form_and_edge():
    cs = A.matrix()
    fast = [c for c in cs if c.family == "fast_fwd"]
    assert {(c.H, c.D, c.mask) for c in fast if c.rep == 1} == {(h, d, k) for h in (256, 512, 768, 1024)
                                                                 for d in (2048, 4096) for k in (False, True)}
    assert {c.R for c in fast} == set(A.FAST_R) and {c.rep for c in fast} == {1, 2, 5}
    gen = [c for c in cs if c.family == "generic"]
    assert {c.rep for c in gen} == set(range(1, 9))
    assert {4, 12, 300, 1028, 2048} <= {c.H for c in gen} and {4, 24, 1024, 2052, 6144} <= {c.D for c in gen}
    assert {41, 63, 64, 65, 100, 129, 1024} <= {c.R for c in gen}
    fb = [c for c in cs if c.family == "fast_bwd"]
    assert {(c.D, c.rep, c.R) for c in fb} == {(d, r, R) for d in (2048, 1024) for r in (1, 5) for R in A.FAST_BWD_R}
    assert {(c.D, c.rep, c.mask) for c in fb} == {(d, r, k) for d in (2048, 1024) for r in (1, 5) for k in (False, True)}
    assert {c.R for c in cs if c.family == "d1024" and c.rep == 5} == set(A.D1024_R)
    assert {c.kind for c in cs if c.family == "edge"} == set(A.KINDS)
    for c in cs:
        if c.nb is None:
            assert set(A.nb_cycle(c.B, c.R).tolist()) == {min(max(x, 1), c.R) for x in (1, 2, c.R - 1, c.R)}, c.id()
