"""CPU pins of the float64 reference of the pre-training steps' bf16 mode (tests/pretrain_bf16_ref.py): with the rounding
off it is oracle.pretrain_oracle.torch_loss_and_grads, and every tolerance the GPU test uses is at most a tenth of what a
step that ignored the flag would show."""
import numpy as np
import pytest

from oracle import pretrain_oracle as PO
from tests import bf16_ref as BR
from tests import pretrain_bf16_ref as R

IDS = ["%s-%s" % (n, "shared" if s else "persite") for n, s in R.WHOLE_STEP_CASES]


@pytest.mark.parametrize("name,ln_shared", R.WHOLE_STEP_CASES, ids=IDS)
def test_with_rounding_off_the_step_is_the_oracle(name, ln_shared):
    """the stacked restatement against the per-head composition of the oracle, float64 both: summation order only"""
    p, batch, masks, d = R.make_case(name, ln_shared)
    assert PO.ln_shared_in(p) == ln_shared
    loss, losses, mid, grads, slices = R.loss_and_grads(p, batch, masks, d["n"], rounding=False)
    tloss, tlosses, tgrads, tslices = PO.torch_loss_and_grads(R.to64(p), R.to64(batch), R.to64(masks), d["n"])
    assert abs(loss - tloss) <= 1e-10 * max(1, abs(tloss))
    assert list(losses) == list(tlosses)
    for k in losses:
        assert abs(losses[k] - tlosses[k]) <= 1e-10 * max(1, abs(tlosses[k])), k
    assert set(grads) == set(tgrads)
    for k in grads:
        np.testing.assert_allclose(grads[k], tgrads[k], rtol=1e-7, atol=1e-11, err_msg=k)
    for k in tslices:
        np.testing.assert_allclose(slices[k], tslices[k], rtol=1e-7, atol=1e-12, err_msg=k)
    # the logits are the oracle's NumPy forward's, head by head
    _, _, omid = PO.forward(R.to64(p), R.to64(batch), R.to64(masks), d["n"])
    Bn = d["B"] * d["n"]
    for h, key in enumerate(("obj/bf_logit", "attr/bf_logit", "obj/ws_logit", "attr/ws_logit")):
        np.testing.assert_allclose(mid["z"][h * Bn:(h + 1) * Bn], omid[key].reshape(Bn, -1), rtol=1e-9, atol=1e-11, err_msg=key)
    # and the rounding is really on otherwise
    assert R.loss_and_grads(p, batch, masks, d["n"], rounding=True)[0] != loss


@pytest.mark.parametrize("name,ln_shared", R.WHOLE_STEP_CASES, ids=IDS)
def test_tolerances_are_a_tenth_of_a_step_that_ignored_the_flag(name, ln_shared):
    """R.tolerances is min(the f32 step's bound, flag distance / 10), so `tolerance <= distance / 10` holds by
    construction and is restated here only as a guard against an edit of that rule.  What this test really pins: no
    tolerance exceeds the bound tests/test_gpu_pretrain.py holds the f32 step to, none is below R.TOL_FLOOR (a witnessed f32
    step can meet it), and the distances themselves are printed.  The per-head report losses are outside: the GPU test
    holds them at the f32 bound, which does not separate the flag on from the flag off (see R.F32_REPORT_TOL)."""
    dist, tol = R.flag_distance(name, ln_shared), R.tolerances(name, ln_shared)
    assert set(dist) == set(tol) and {"loss", "logit", "sq", "grad/classifier/fc/weights", "grad/L_GloVe/embed_map"} <= set(dist)
    for q in sorted(dist):
        print("%-10s %-60s distance %.3e  tolerance %.3e" % (name, q, dist[q], tol[q]))
    for q in dist:
        assert tol[q] <= dist[q] / 10, (q, dist[q], tol[q])          # distance >= 10 x tolerance
        assert tol[q] >= R.TOL_FLOOR, (q, tol[q])                 # ... and a witnessed f32 step can meet it
    assert tol["logit"] <= R.F32_LOGIT_TOL and tol["loss"] <= R.F32_REPORT_TOL
    assert all(tol[q] <= R.F32_GRAD_TOL for q in tol if q.startswith("grad/"))
    assert BR.WITNESS_TOL == 2e-4


def test_a_witness_of_the_reference_itself_changes_nothing():
    """the witnessed mode fed with this reference's own routed operands in float32: the logged distances are f32
    rounding, and loss and gradients stay within the whole-step tolerances"""
    p, batch, masks, d = R.make_case("medium")
    l0, _, m0, g0, _ = R.loss_and_grads(p, batch, masks, d["n"])
    assert set(m0["routed"]) == set(R.ROUTED)
    Bn, H = d["B"] * d["n"], d["H"]
    assert m0["routed"]["pooled_linear_l"]["x"].shape == (2 * Bn, d["D"]) and m0["routed"]["pooled_linear_l"]["d"].shape == (2 * Bn, H)
    assert m0["routed"]["classifier"]["x"].shape == (4 * Bn, 2 * H) and m0["routed"]["classifier"]["d"].shape == (4 * Bn, d["A"])
    wit = {k: {"x": v["x"].astype(np.float32), "d": v["d"].astype(np.float32)} for k, v in m0["routed"].items()}
    l1, _, m1, g1, _ = R.loss_and_grads(p, batch, masks, d["n"], witness=wit)
    tol = R.tolerances("medium")
    for k in R.ROUTED:
        assert 0 <= wit[k]["log"]["x"] <= 1e-7 and 0 < wit[k]["log"]["d"] <= 1e-7, (k, wit[k]["log"])
    assert abs(l1 - l0) <= tol["loss"] * max(1, abs(l0))
    for q in tol:
        if q.startswith("grad/"):
            assert R.grad_distance(g1[q[5:]], g0[q[5:]]) <= tol[q], q
    wit["classifier"]["x"] = wit["classifier"]["x"] * np.float32(1.01)
    R.loss_and_grads(p, batch, masks, d["n"], witness=wit)
    assert wit["classifier"]["log"]["x"] > BR.WITNESS_TOL


def test_the_summed_d_pre_of_pooled_linear_l_is_rounded_once():
    """both heads of a category read ONE pooled_linear_l pre-activation, so dW = r(x)^T r(d_bf + d_ws), not the sum of two
    rounded products: the routed tape's d is the sum and reproduces the weight gradient through gemm_ref"""
    import torch
    p, batch, masks, d = R.make_case("toy")
    _, _, mid, grads, _ = R.loss_and_grads(p, batch, masks, d["n"])
    for layer in R.ROUTED:
        x, dp = (torch.from_numpy(mid["routed"][layer][s]) for s in ("x", "d"))
        want = BR.round_bf16(x).t() @ BR.round_bf16(dp)
        np.testing.assert_allclose(grads[layer + "/fc/weights"], want.numpy(), rtol=1e-12, atol=1e-18, err_msg=layer)
