"""tests/loss_ref.py itself (CPU): the references against the project's oracles and torch's own losses, torch.amin's
gradient over ties, the RT table against the live measurement, the float32 evaluations inside their bounds, the case
matrix against a restatement of the dispatch conditions (every route has a case), and the mutants the judges must
catch."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pretrain_oracle as PO
from oracle import vqa_oracle as O
from tests import loss_ref as L
from tests import rowop_ref as R

F64 = torch.float64


def _np(t):
    return t.double().numpy()


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


# ----------------------------------------------------------------------------------------------------- against oracles
@pytest.mark.parametrize("A", [3, 65, 257])
@pytest.mark.parametrize("model,utm", [("vlmap_answer", 1), ("standard", 0)])
def test_loss_fwd_reproduces_the_oracle(A, model, utm):
    d = L.loss_inputs(A, 0, "random")
    ref = L.sigmoid_loss(d["z"], d["tgt"], d["masks"], 0, utm, 1.0 / L.LOSS_B)
    am = {k: _np(v) for k, v in d["masks"].items()}
    loss, report, out, ell = O.loss_and_report(_np(d["z"]), _np(d["tgt"]), am, model)
    rep, _ = R.report_reduce(ref["stats"])
    _close(rep.numpy(), list(report.values()))
    assert np.array_equal(ref["pred"].numpy(), out["pred"])
    _close(ref["stats"][:, R.S_MAX_TRAIN].numpy(), out["max_train_score"])
    _close(ref["stats"][:, R.S_TEST_OBJ_MAX].numpy(), out["test_obj_max_score"])
    _close(ref["stats"][:, R.S_LOSS_REPORT].numpy(), ell.sum(1))
    assert float(ref["stats"][:, 15].abs().max()) == 0.0
    # autograd of torch's own loss
    x = d["z"].double().requires_grad_(True)
    w = d["masks"]["train"].double() if utm else torch.ones(A, dtype=F64)
    bce = F.binary_cross_entropy_with_logits(x, d["tgt"].double(), reduction="none")
    (g,) = torch.autograd.grad((bce * w).sum() / L.LOSS_B, x)
    _close(ref["dz"].numpy(), g.numpy())
    _close(ref["stats"][:, R.S_LOSS_REPORT].numpy(), bce.detach().sum(1).numpy())


@pytest.mark.parametrize("A", [3, 65, 257])
@pytest.mark.parametrize("form", [1, 2])
def test_loss2_fwd_reproduces_the_two_headed_oracles(A, form):
    d = L.loss_inputs(A, form, "random")
    ref = L.sigmoid_loss(d["z"], d["tgt"], d["masks"], form, 1, 1.0 / L.LOSS_B, d["z2"])
    am = {k: _np(v) for k, v in d["masks"].items()}
    fn = O.loss_and_report_all2 if form == 1 else O.loss_and_report_all1
    loss, report, out = fn(_np(d["z"]), _np(d["z2"]), _np(d["tgt"]), am)
    rep, _ = R.report_reduce(ref["stats"])
    # sum_mode 1 takes the CE of the float32 sum, the oracle of the float64 one: |z| 2^-24 per logit
    _close(rep.numpy(), list(report.values()), 1e-12 if form == 1 else 1e-6)
    assert np.array_equal(ref["pred"].numpy(), out["pred"])
    assert torch.equal(ref["z_sum"], d["z"] + d["z2"]) and ref["z_sum"].dtype == torch.float32
    # the gradients against torch's own loss
    x, x2 = (t.double().requires_grad_(True) for t in (d["z"], d["z2"]))
    t, tr = d["tgt"].double(), d["masks"]["train"].double()
    bce = lambda v: F.binary_cross_entropy_with_logits(v, t, reduction="none")
    total = (bce(x) * tr + bce(x2)).sum() if form == 1 else ((bce(x) + bce(x + x2)) * tr).sum()
    g, g2 = torch.autograd.grad(total / L.LOSS_B, (x, x2))
    _close(ref["dz"].numpy(), g.numpy(), 1e-12 if form == 1 else 1e-6)
    _close(ref["dz2"].numpy(), g2.numpy(), 1e-12 if form == 1 else 1e-6)


def test_planted_ties_are_ties_and_the_first_index_wins():
    for form in (0, 1, 2):
        for A in (65, 257, 513, 3000):
            d = L.loss_inputs(A, form, "random")
            ref = L.sigmoid_loss(d["z"], d["tgt"], d["masks"], form, 1, 1.0, d["z2"])
            cmp32 = d["z"] if form == 0 else (d["z"] + d["z2"] if form == 2 else
                                              d["z"] * (1 - d["masks"]["train"]) + d["z2"] * d["masks"]["train"])
            assert len(d["ties"]) == (3 if form == 0 else 4)
            for row, i, j in d["ties"]:
                assert i < j and float(cmp32[row, i]) == float(cmp32[row, j]) == float(cmp32[row].max())
                assert int(ref["pred"][row]) == i
            assert int(ref["pred"][0]) == 0 and int(ref["pred"][4]) == A - 1
            if form:    # the tie of row 5 is in neither head
                _, i, j = d["ties"][-1]
                assert float(d["z"][5, i]) != float(d["z"][5, j]) and float(d["z2"][5, i]) != float(d["z2"][5, j])


def test_masked_maxima_of_empty_masks_are_zero():
    for kind in ("zeros", "ones"):
        d = L.loss_inputs(257, 0, kind)
        s = L.sigmoid_loss(d["z"], d["tgt"], d["masks"], 0, 1, 1.0)["stats"]
        if kind == "zeros":     # train = 0: every answer is a test answer; obj = attr = exist = 0
            assert float(s[:, [R.S_MAX_EXIST, R.S_MAX_TRAIN_EXIST, R.S_TEST_OBJ_MAX, R.S_MAX_TRAIN]].abs().max()) == 0.0
            assert float(s[:, R.S_LOSS_TRAIN].abs().max()) == 0.0 and float(s[:, R.S_TEST_MAX].min()) > 0.0
        else:                   # train = 1: no test answers
            assert float(s[:, [R.S_TEST_MAX, R.S_TEST_OBJ_MAX, R.S_TEST_ATTR_MAX, R.S_TEST_MAX_EXIST]].abs().max()) == 0.0
            assert torch.equal(s[:, R.S_LOSS_TRAIN], s[:, R.S_LOSS_REPORT])
        assert bool(torch.isfinite(s).all())


@pytest.mark.parametrize("A,topk", [(8, 5), (37, 5), (1028, 5), (37, 1)])
def test_softmax_ce_reproduces_the_oracle_and_torch(A, topk):
    d = L.softmax_inputs(A, topk, "most")
    ref = L.softmax_ce(d["z"], d["label"], d["valid"], topk, d["inv"])
    s = ref["stats"].sum(0) * d["inv"]
    if topk == PO.TOP_K:
        loss, acc, hit = PO.n_way_classification_loss(_np(d["z"])[None], d["label"].long().numpy()[None], _np(d["valid"])[None])
        _close(s[:3].numpy(), [loss, acc, hit], 1e-12)
    x = d["z"].double().requires_grad_(True)
    ce = F.cross_entropy(x, d["label"].long(), reduction="none")
    (g,) = torch.autograd.grad((ce * d["valid"].double()).sum() * d["inv"], x)
    _close(ref["dz"].numpy(), g.numpy())
    _close(ref["stats"][:, 0].numpy(), (ce.detach() * d["valid"].double()).numpy(), 1e-12)
    assert float(ref["dz"][7].abs().max()) == 0.0 and float(ref["stats"][7].abs().max()) == 0.0
    # the planted ranks: rows 3 and 5 are hits at rank topk - 1, rows 4 and 6 misses at rank topk
    rank = L.rank_of_label(d["z"], d["label"])
    assert rank[3:7].tolist() == [topk - 1, topk, topk - 1, topk]
    assert ref["stats"][3:7, 2].tolist() == [1.0, 0.0, 1.0, 0.0]
    assert ref["stats"][2, 1] == 0.0 and int(rank[2]) == 1          # the label is the second of two tied maxima
    # a SUM head is the CE of the float32 sum
    z2 = torch.from_numpy(np.random.default_rng(3).standard_normal(d["z"].shape).astype(np.float32))
    a = L.softmax_ce(d["z"], d["label"], d["valid"], topk, d["inv"], z2)
    b = L.softmax_ce(d["z"] + z2, d["label"], d["valid"], topk, d["inv"])
    assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["dz"], b["dz"])


def test_amin_autograd_splits_evenly_over_ties():
    for A, kind in ((257, "random"), (3000, "random"), (3, "zeros"), (257, "ones")):
        d = L.rowmin_inputs(A, kind)
        g, _ = L.rowmin_mask_bwd(d["dz"], d["z"], d["exist"])
        dz, z, e = d["dz"].double(), d["z"].double(), d["exist"].double()
        tie = (z == z.amin(1, keepdim=True)).double()
        cnt = tie.sum(1, keepdim=True)
        if kind == "random":
            assert cnt[:6, 0].tolist() == [1, 1, 2, 3, A, 2]
        want = dz * e + tie * (dz * (1 - e)).sum(1, keepdim=True) / cnt
        _close(g.numpy(), want.numpy(), 1e-14)
        # the same gradient from the plain form z exist + amin(z) (1 - exist)
        x = z.clone().requires_grad_(True)
        zm, _ = L.rowmin_mask_fwd(x, d["exist"])
        (g2,) = torch.autograd.grad((dz * zm).sum(), x)
        _close(g2.numpy(), want.numpy(), 1e-12)
    # finite differences on the rows without ties
    d = L.rowmin_inputs(65, "random")
    g, _ = L.rowmin_mask_bwd(d["dz"], d["z"], d["exist"])
    f = lambda zz: float((d["dz"].double() * L.rowmin_mask_fwd(zz, d["exist"])[0]).sum())
    z = d["z"].double()
    for row in (0, 1, 6):
        for a in (65 // 3, (2 * 65) // 3, 7):
            hi, lo = z.clone(), z.clone()
            hi[row, a] += 1e-6
            lo[row, a] -= 1e-6
            assert abs((f(hi) - f(lo)) / 2e-6 - float(g[row, a])) < 1e-6


def test_rowmin_forward_is_exact_in_float32():
    d = L.rowmin_inputs(257, "random")
    zm, m = L.rowmin_mask_fwd(d["z"], d["exist"])
    want = torch.where(d["exist"][None, :] != 0, d["z"], d["z"].amin(1, keepdim=True))
    assert torch.equal(zm.float(), want) and torch.equal(zm, want.double()) and torch.equal(m.float(), d["z"].amin(1))


def test_ln_pair_mul_is_two_layer_norms_and_a_product():
    rng = np.random.default_rng(5)
    pa, ga, ba = L.ln_inputs(5, 16, rng)
    pb, gb, bb = L.ln_inputs(5, 16, rng)
    f = L.ln_pair_mul_fwd(pa, pb, ga, ba, gb, bb)
    ln, _, _ = O.layer_norm_forward(_np(pa), _np(ga), _np(ba))
    _close(f["y_a"].numpy(), np.maximum(ln, 0))
    dz, add = (torch.from_numpy(rng.standard_normal((5, 16)).astype(np.float32)) for _ in range(2))
    b = L.ln_pair_mul_bwd(dz, add, pa, pb, ga, ba, gb, bb)
    # one autograd pass through the whole pair
    xa, xb = (t.double().requires_grad_(True) for t in (pa, pb))
    ya = torch.relu(F.layer_norm(xa, (16,), ga.double(), ba.double(), eps=R.LN_EPS))
    yb = torch.relu(F.layer_norm(xb, (16,), gb.double(), bb.double(), eps=R.LN_EPS))
    g = torch.autograd.grad((dz.double() * ya * yb).sum() + (add.double() * yb).sum(), (xa, xb))
    _close(b["dpre_a"].numpy(), g[0].numpy(), 1e-9)
    _close(b["dpre_b"].numpy(), g[1].numpy(), 1e-9)
    _close(b["part_dbias_b"].numpy(), g[1].numpy(), 1e-9)
    none = L.ln_pair_mul_bwd(dz, None, pa, pb, ga, ba, gb, bb)
    zero = L.ln_pair_mul_bwd(dz, torch.zeros_like(dz), pa, pb, ga, ba, gb, bb)
    assert all(torch.equal(none[k], zero[k]) for k in none)


# ------------------------------------------------------------------------------------------------------ RT and routes
@pytest.fixture(scope="module")
def measured():
    return L.measure_rt(L.RT)


def test_rt_table_is_the_live_measurement(measured):
    for what, (worst, at) in measured.items():
        want, where = L.MEASURED[what]
        assert abs(worst - want) <= 0.01 * want, (what, worst, at)
        assert at == where, (what, at)
        assert abs(L.RT[what] - 8 * want) <= 1e-12
        row = re.search(r"^  %s +(\S+) +(\S+) +(.+)$" % what, L.__doc__, re.M)
        assert row and abs(float(row.group(1)) - want) <= 0.01 * want and abs(float(row.group(2)) - 8 * want) <= 0.01 * 8 * want
        assert row.group(3).strip() == where


def test_float32_evaluations_are_inside_the_bound(measured):
    # the fixture raised if one was outside RT x scale; they are at most 1/8 of it
    for what, (worst, at) in measured.items():
        assert 0 < worst <= L.RT[what] / 8 * 1.01, (what, at)
    rng = np.random.default_rng(9)
    for N in (16, 1028, 4096):
        pa, ga, ba = L.ln_inputs(5, N, rng)
        pb, gb, bb = L.ln_inputs(5, N, rng)
        dz, add = (torch.from_numpy(rng.standard_normal((5, N)).astype(np.float32)) for _ in range(2))
        L.judge_ln_pair_fwd(L.ln_pair_mul_fwd(pa, pb, ga, ba, gb, bb, torch.float32),
                            L.ln_pair_mul_fwd(pa, pb, ga, ba, gb, bb), pa, pb, "N=%d" % N)
        L.judge_ln_pair_bwd(L.ln_pair_mul_bwd(dz, add, pa, pb, ga, ba, gb, bb, torch.float32),
                            L.ln_pair_mul_bwd(dz, add, pa, pb, ga, ba, gb, bb), "N=%d" % N)
    for name, (A, heads) in L.pair_cases().items():
        for h, head in enumerate(L.pair_inputs(A, heads)):
            got = {}
            for sname, dnames, r in L.pair_tasks(head, 5, torch.float32):
                got[sname] = r["stats"]
                got.update({dn: r["dz"] for dn in dnames})
            got.setdefault("stats_l", torch.full((3, 4), float("nan")))
            L.judge_pair_head(got, head, 5, "%s head %d" % (name, h))


def test_the_matrix_reaches_every_route():
    reached = {}
    for c in L.loss_cases():
        entry = "loss_fwd" if c[1] == 0 else "loss2_fwd"
        reached.setdefault(("loss form", L.loss_kernel_form(entry, c[1] == 2)), L.loss_id(*c))
    for A, topk, vk in L.softmax_cases():
        for fast, zo, do in L.softmax_variants(A):
            route = L.softmax_route(A, fast, not (zo or do))
            name = "%s fast %d z+%d dz+%d" % (L.softmax_id(A, topk, vk), fast, zo, do)
            reached.setdefault(("single", route), name)
            if fast and (zo or do) and L.softmax_route(A, fast, True) != "three-pass":
                reached.setdefault(("single", "three-pass by misalignment", "z" if zo else "dz"), name)
    for name, (A, heads) in L.pair_cases().items():
        aligned = all(m is None for _, m in heads)
        route = L.softmax_route(A, 1, aligned)
        for split, _ in heads:
            reached.setdefault(("SPLIT" if split else "SUM", route), name)
            if not aligned and L.softmax_route(A, 1, True) != "three-pass":
                reached.setdefault(("SPLIT" if split else "SUM", "three-pass by misalignment"), name)
    for N in L.LN_N:
        reached.setdefault(("ln_pair_mul VPT", L.ln_pair_vpt(N)), "N=%d" % N)
    want = [("loss form", f) for f in (0, 1, 2)]
    want += [(k, r) for k in ("single", "SPLIT", "SUM") for r in ("three-pass", 1, 2, 3, 4)]
    want += [("single", "three-pass by misalignment", "z"), ("single", "three-pass by misalignment", "dz"),
             ("SPLIT", "three-pass by misalignment"), ("SUM", "three-pass by misalignment")]
    want += [("ln_pair_mul VPT", v) for v in (1, 2, 4)]
    missing = [w for w in want if w not in reached]
    assert not missing, missing
    print("\n".join("  %-50s %s" % (" ".join(str(x) for x in w), reached[w]) for w in want))
    # the restated conditions at their edges
    assert [L.softmax_route(A) for A in (4, 1024, 1028, 2048, 2052, 3072, 3076, 4096)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert L.softmax_route(4100) == L.softmax_route(1020, 0) == L.softmax_route(37) == "three-pass"
    assert [L.ln_pair_vpt(N) for N in (4, 1024, 1028, 2048, 2052, 4096, 4100, 1022)] == [1, 1, 2, 2, 4, 4, None, None]
    assert any(len(h) == L.PAIR_MAX for _, h in L.pair_cases().values())


# ------------------------------------------------------------------------------------------------------------- mutants
def _as_got(ref, keys):
    return {k: (ref[k].float() if ref[k] is not None and ref[k].dtype.is_floating_point else ref[k]) for k in keys}


LOSS_KEYS = ("stats", "pred", "dz", "dz2", "z_sum")


@pytest.mark.parametrize("form,tamper", [(0, "last_tie"), (1, "last_tie"), (2, "last_tie"), (2, "sum_term_unmasked"),
                                         (1, "pred_from_sum")])
def test_the_loss_judge_catches(form, tamper):
    d = L.loss_inputs(257, form, "random")
    kw = dict(form=form, use_train_mask=1, inv_batch=1.0 / L.LOSS_B, z2=d["z2"])
    ref = L.sigmoid_loss(d["z"], d["tgt"], d["masks"], **kw)
    L.judge_loss(_as_got(ref, LOSS_KEYS), ref, "unchanged")
    bad = L.sigmoid_loss(d["z"], d["tgt"], d["masks"], tamper=(tamper,), **kw)
    with pytest.raises(AssertionError):
        L.judge_loss(_as_got(bad, LOSS_KEYS), ref, tamper)
    if tamper == "sum_term_unmasked":       # each output on its own catches it
        for keys in (("stats", "pred"), ("stats", "pred", "dz"), ("stats", "pred", "dz2")):
            got = _as_got(ref, ("stats", "pred"))
            got.update(_as_got(bad, keys[2:]) if len(keys) > 2 else {"stats": bad["stats"].float()})
            with pytest.raises(AssertionError):
                L.judge_loss(got, ref, tamper)


def test_the_rowmin_judge_catches_an_unsplit_gradient():
    d = L.rowmin_inputs(257, "random")
    ref, scale = L.rowmin_mask_bwd(d["dz"], d["z"], d["exist"])
    args = (scale, d["dz"], d["z"], d["exist"])
    L.judge_rowmin_bwd(ref.float(), ref, *args, "unchanged")
    bad, _ = L.rowmin_mask_bwd(d["dz"], d["z"], d["exist"], tamper=("whole_to_every_tie",))
    assert torch.equal(bad[0], ref[0]) and not torch.equal(bad[2], ref[2])
    with pytest.raises(AssertionError):
        L.judge_rowmin_bwd(bad.float(), ref, *args, "whole_to_every_tie")
    keep = (d["exist"][None, :] == 1) & (d["z"] != d["z"].amin(1, keepdim=True))
    row, col = (int(v) for v in keep.nonzero()[0])
    got = ref.float()
    got[row, col] = torch.nextafter(got[row, col], torch.tensor(float("inf")))
    with pytest.raises(AssertionError):     # an existing answer's gradient must keep its bits
        L.judge_rowmin_bwd(got, ref, *args, "one ulp")


@pytest.mark.parametrize("A,tamper", [(37, "last_tie"), (37, "rank_ge"), (37, "no_inv_scale"), (37, "invalid_rows_written"),
                                      (1028, "padding_lane"), (2052, "padding_lane")])
def test_the_softmax_judge_catches(A, tamper):
    d = L.softmax_inputs(A, 5, "most")
    ref = L.softmax_ce(d["z"], d["label"], d["valid"], 5, d["inv"])
    L.judge_softmax(_as_got(ref, ("stats", "dz")), ref, "unchanged")
    bad = L.softmax_ce(d["z"], d["label"], d["valid"], 5, d["inv"], tamper=(tamper,))
    with pytest.raises(AssertionError):
        L.judge_softmax(_as_got(bad, ("stats", "dz")), ref, tamper)


def test_the_pair_judge_catches_a_sum_head_that_writes_one_block():
    A, heads = L.pair_cases()["pair-A40-mixed"]
    head = L.pair_inputs(A, heads)[0]
    assert head["split"] == 0
    (_, _, r), = L.pair_tasks(head, 5)
    nan = lambda *s: torch.full(s, float("nan"))
    got = dict(stats_v=r["stats"].float(), stats_l=nan(3, 4), dzv=r["dz"].float(), dzl=r["dz"].float())
    L.judge_pair_head(got, head, 5, "unchanged")
    with pytest.raises(AssertionError):
        L.judge_pair_head(dict(got, dzl=nan(3, A)), head, 5, "dzl not written")
    with pytest.raises(AssertionError):
        L.judge_pair_head(dict(got, stats_l=torch.zeros(3, 4)), head, 5, "stats_l written")
    with pytest.raises(AssertionError):     # the CE of zv alone instead of zv + zl
        alone = L.softmax_ce(head["zv"], head["label"], head["valid"], 5, head["inv"])
        L.judge_pair_head(dict(got, stats_v=alone["stats"].float(), dzv=alone["dz"].float(), dzl=alone["dz"].float()),
                          head, 5, "zv alone")


def test_the_ln_pair_judge_catches_add_b_on_the_wrong_side():
    rng = np.random.default_rng(11)
    pa, ga, ba = L.ln_inputs(5, 1028, rng)
    pb, gb, bb = L.ln_inputs(5, 1028, rng)
    dz, add = (torch.from_numpy(rng.standard_normal((5, 1028)).astype(np.float32)) for _ in range(2))
    ref = L.ln_pair_mul_bwd(dz, add, pa, pb, ga, ba, gb, bb)
    L.judge_ln_pair_bwd({k: v.float() for k, v in ref.items()}, ref, "unchanged")
    bad = L.ln_pair_mul_bwd(dz, add, pa, pb, ga, ba, gb, bb, tamper=("add_b_on_a",))
    for k in ("dpre_a", "dpre_b", "part_dbeta_b", "part_dbias_a"):
        with pytest.raises(AssertionError):
            L.judge_ln_pair_bwd({k: bad[k].float()}, ref, "add_b_on_a")
