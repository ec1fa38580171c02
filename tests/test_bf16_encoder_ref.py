"""CPU pins of the reference of the bf16 VQA step with routed encoder products (tests/bf16_encoder_ref.py): with the
encoder rounding off it is tests/bf16_ref.py, and with it on it sits at least 10 x the UNCHANGED tolerances of bf16_ref.py
from it on every quantity the flag moves -- so those tolerances tell FusionEngine(encoder="bf16-gemms") from
encoder="f32".  The `small` case is left out: at H 16, W 12, T 7 its logits do not move at all."""
import numpy as np
import pytest

from oracle import vqa_oracle as O
from tests import bf16_encoder_ref as E
from tests import bf16_ref as R
from tests.gpu_util import make_case

MED = [c for c in R.MODEL_CASES if c[0] == "med"][0]
MED_B64 = ("med", MED[1], 64) + MED[3:]


@pytest.mark.parametrize("model_type", R.MODEL_TYPES)
def test_without_encoder_rounding_it_is_bf16_ref(model_type):
    name, dims, B, Rg, T, N = R.MODEL_CASES[0]
    p, table, nbox, batch, am, masks = make_case(R.MODEL_SEED, model_type, B, Rg, T, N, dims)
    pp = {k: v for k, v in p.items() if not O.is_const(k)}
    want = R.loss_and_grads(pp, batch, table, nbox, am, masks, model_type)
    got = E.loss_and_grads(pp, batch, table, nbox, am, masks, model_type, enc_rounding=False)
    assert R._gru.__name__ == "_gru"                              # the replacement is gone again
    assert abs(got[0] - want[0]) <= 1e-12
    np.testing.assert_allclose(got[1]["logit"], want[1]["logit"], rtol=0, atol=1e-12)
    assert set(got[2]) == set(want[2])
    for k, v in want[2].items():
        assert np.abs(got[2][k] - v).max() <= 1e-12 * max(1.0, np.abs(v).max()), k
    assert np.abs(got[3] - want[3]).max() <= 1e-12 * max(1.0, np.abs(want[3]).max())
    assert got[4] == pytest.approx(want[4], abs=1e-12)
    # and the encoder rounding is really on otherwise
    on = E.loss_and_grads(pp, batch, table, nbox, am, masks, model_type)
    assert any(np.abs(on[2][k] - want[2][k]).max() > 0 for k in E.gru_names(model_type))


@pytest.mark.parametrize("model_type", R.MODEL_TYPES)
@pytest.mark.parametrize("case", [MED, MED_B64], ids=["med", "med-B64"])
def test_encoder_rounding_is_visible_at_ten_times_the_tolerances(model_type, case):
    (l0, m0, g0, dx0, _), (l1, m1, g1, dx1, _) = E.reference_pair(model_type, case)
    dist = {k: R.grad_distance(g1[k], g0[k]) for k in E.gru_names(model_type)}
    dist["dx_embed"] = R.grad_distance(dx1, dx0)
    d_logit = float(np.abs(m1["logit"] - m0["logit"]).max())
    for k, v in dist.items():
        print("%s B %d  %-50s encoder-rounded vs plain %.3e  (x %.0f GRAD_TOL)" % (model_type, case[2], k, v, v / R.GRAD_TOL))
    print("%s B %d  logits %.3e  (x %.0f LOGIT_TOL)" % (model_type, case[2], d_logit, d_logit / R.LOGIT_TOL))
    assert all(v >= 10 * R.GRAD_TOL for v in dist.values()), dist
    assert d_logit >= 10 * R.LOGIT_TOL, d_logit


def test_a_witness_of_the_reference_itself_changes_nothing():
    """the witnessed mode fed with this reference's own tapes in float32: the logged distances are f32 rounding and loss
    and gradients move by no more than a few flips; a witness far from the reference's own value shows in the log"""
    name, dims, B, Rg, T, N = MED
    mt = "standard"
    p, table, nbox, batch, am, masks = make_case(R.MODEL_SEED, mt, 8, Rg, T, 16, dims)
    pp = {k: v for k, v in p.items() if not O.is_const(k)}
    l0, m0, g0, dx0, _, enc0 = E.loss_and_grads(pp, batch, table, nbox, am, masks, mt)
    wit = {k: v.astype(np.float32) for k, v in enc0.tape().items()}
    l1, m1, g1, dx1, _, enc1 = E.loss_and_grads(pp, batch, table, nbox, am, masks, mt, enc_witness=wit)
    assert len(enc1.logs) == 1 + 2 * T and all(set(lg) == {"x", "d"} for lg in enc1.logs)
    assert 0 < enc1.witness_distance() <= 1e-6, enc1.witness_distance()
    assert abs(l1 - l0) <= R.LOSS_TOL * max(1, abs(l0))
    for k in O.train_var_names(pp, mt):
        if not k.endswith("score/fc/biases"):
            assert R.grad_distance(g1[k], g0[k]) <= R.GRAD_TOL, k
    assert R.grad_distance(dx1, dx0) <= R.GRAD_TOL
    wit["rh"] = wit["rh"] * np.float32(1.01)
    enc2 = E.loss_and_grads(pp, batch, table, nbox, am, masks, mt, enc_witness=wit)[-1]
    assert enc2.witness_distance() > R.WITNESS_TOL
