"""CPU checks of the adapted-memory pre-training model's float64 reference (tests/pretrain_adapt_ref.py) and of its host
side: model registry, variable names and shapes, LayerNorm slots, report keys, and that the variables of every model
type that existed before it are what they were (tests/golden/pretrain_variable_shapes.json)."""
import json
import os

import numpy as np
import pytest

from oracle import pretrain_oracle as PO
from tests import pretrain_adapt_ref as AR

DIMS = dict(B=3, n=5, R=6, D=10, H=6, L=4, W=8, Vq=20, n_ws=7, A=12)


def _case(seed=0, ln_shared=True, adapt=True, dims=DIMS):
    d = dims
    rng = np.random.default_rng(seed)
    p = AR.init_params(rng, d["Vq"], d["n_ws"], d["A"], W=d["W"], D=d["D"], H=d["H"], ln_shared=ln_shared, adapt=adapt,
                       dtype=np.float64)
    b = PO.make_batch(rng, d["B"], d["n"], d["R"], d["D"], d["L"], d["Vq"], d["n_ws"], d["A"], dtype=np.float64)
    m = PO.make_masks(rng, d["B"], d["n"], d["R"], d["H"], dtype=np.float64)
    return p, b, m


@pytest.mark.parametrize("ln_shared", [True, False])
def test_numpy_forward_equals_torch(ln_shared):
    p, b, m = _case(2, ln_shared)
    total, rep, mid = AR.forward(p, b, m, 5)
    tt, losses, g, sl = AR.torch_loss_and_grads(p, b, m, 5)
    assert abs(tt - total) <= 1e-10 * abs(total)
    assert list(rep) == AR.report_keys() and len(rep) == 13
    for name, v in losses.items():
        assert abs(rep[name + "_loss"] - v) <= 1e-10 * max(1.0, abs(v)), name
    assert mid["obj/pooled_V_ft"].shape == (3, 5, 6) and mid["obj/va"].shape == (3, 6, 6)
    assert np.array_equal(mid["obj/va"], mid["attr/va"]) == ln_shared      # one memory, or one per call site
    cap = {}
    AR.torch_loss_and_grads(p, b, m, 5, capture=cap)
    assert set(cap) == set(AR.relu_sites()) and cap["obj/va"].shape == (3, 6, 6)
    _, _, gg, _ = AR.torch_loss_and_grads(p, b, m, 5, gates=cap)
    for k in g:
        assert np.abs(gg[k] - g[k]).max() <= 1e-12 * max(np.abs(g[k]).max(), 1e-30), k


@pytest.mark.parametrize("ln_shared", [True, False])
def test_finite_differences_of_the_adapt_variables(ln_shared):
    """torch autograd of v_adapt (weights, biases, LayerNorm) and of the [H, H] pooled_linear_l against central
    differences of the NumPy forward"""
    p, b, m = _case(3, ln_shared)
    _, _, g, _ = AR.torch_loss_and_grads(p, b, m, 5)
    rng = np.random.default_rng(7)
    eps = 1e-6
    names = ["v_adapt/fc/weights", "v_adapt/fc/biases", "v_adapt/LayerNorm/gamma", "v_adapt/LayerNorm/beta",
             "pooled_linear_l/fc/weights"] + ([] if ln_shared else ["v_adapt/LayerNorm_1/gamma", "v_adapt/LayerNorm_1/beta"])
    for name in names:
        for _ in range(3):
            idx = tuple(rng.integers(0, s) for s in p[name].shape)
            hi, lo = dict(p), dict(p)
            hi[name], lo[name] = p[name].copy(), p[name].copy()
            hi[name][idx] += eps
            lo[name][idx] -= eps
            fd = (AR.forward(hi, b, m, 5)[0] - AR.forward(lo, b, m, 5)[0]) / (2 * eps)
            assert abs(fd - g[name][idx]) <= 1e-6 * max(1.0, abs(fd)), (name, idx, fd, g[name][idx])


@pytest.mark.parametrize("ln_shared", [True, False])
def test_without_the_adapt_layer_it_is_the_cfg5_oracle(ln_shared):
    """adapt=False: total, report and every gradient equal pretrain_oracle's, which pins everything but the new layer"""
    p, b, m = _case(4, ln_shared, adapt=False)
    assert sorted(p) == sorted(PO.variable_shapes(20, 7, 12, 8, 10, 6, ln_shared))
    total, rep, mid = AR.forward(p, b, m, 5, adapt=False)
    t0, r0, m0 = PO.forward(p, b, m, 5)
    assert total == t0 and rep == r0
    for k in PO.KINDS:
        np.testing.assert_array_equal(mid[k + "/pooled_V_ft"], m0[k + "/pooled_V_ft"])
        np.testing.assert_array_equal(mid[k + "/ws_logit"], m0[k + "/ws_logit"])
    ta, la, ga, sa = AR.torch_loss_and_grads(p, b, m, 5, adapt=False)
    tb, lb, gb, sb = PO.torch_loss_and_grads(p, b, m, 5)
    assert abs(ta - tb) <= 1e-13 * abs(tb) and sorted(la) == sorted(lb)
    for k in gb:
        assert np.abs(ga[k] - gb[k]).max() <= 1e-12 * max(np.abs(gb[k]).max(), 1e-30), k
    for k in sb:
        assert np.abs(sa[k] - sb[k]).max() <= 1e-12 * max(np.abs(sb[k]).max(), 1e-30), k


def test_the_two_easy_mistakes_move_the_total_by_more_than_the_comparison_bar():
    """pooling relu(V_ft W + b) without the LayerNorm, and normalising each region's [H] instead of the image's [R, H]
    block, both change the total loss by more than the GPU comparison's 2e-4 relative bar"""
    from oracle import vqa_oracle as O
    p, b, m = _case(5)
    total, _, _ = AR.forward(p, b, m, 5)

    def no_ln(p_, x, ki):
        return np.maximum(x @ p_["v_adapt/fc/weights"] + p_["v_adapt/fc/biases"], 0)

    def per_region(p_, x, ki):
        pre = x @ p_["v_adapt/fc/weights"] + p_["v_adapt/fc/biases"]
        B, R, H = pre.shape
        ln, _, _ = O.layer_norm_forward(pre.reshape(B * R, H), p_["v_adapt/LayerNorm/gamma"], p_["v_adapt/LayerNorm/beta"])
        return np.maximum(ln.reshape(B, R, H), 0)

    for mutant in (no_ln, per_region):
        t, _, _ = AR.forward(p, b, m, 5, memory=mutant)
        assert abs(t - total) > 2e-4 * max(1.0, abs(total)), (mutant.__name__, t, total)
    t, _, _ = AR.forward(p, b, m, 5, memory=AR.v_adapt)
    assert t == total


def test_per_call_site_layernorm_1_belongs_to_the_attribute_builder():
    p, b, m = _case(6, ln_shared=False)
    _, rep, _ = AR.forward(p, b, m, 5)
    q = dict(p)
    q["v_adapt/LayerNorm_1/gamma"] = p["v_adapt/LayerNorm_1/gamma"] * 1.5
    _, rep2, _ = AR.forward(q, b, m, 5)
    for k in rep:
        if k.startswith("obj_"):
            assert rep2[k] == rep[k], k
    assert rep2["attr_blank_fill_loss"] != rep["attr_blank_fill_loss"]
    assert rep2["attr_wordset_loss"] != rep["attr_wordset_loss"]
    _, _, g, _ = AR.torch_loss_and_grads(p, b, m, 5)
    assert np.abs(g["v_adapt/LayerNorm/gamma"]).max() > 0 and np.abs(g["v_adapt/LayerNorm_1/gamma"]).max() > 0
    assert not np.allclose(g["v_adapt/LayerNorm/gamma"], g["v_adapt/LayerNorm_1/gamma"])


def test_registry_variables_ln_slots_and_report_keys():
    from vqa_transfer_externaldata_amd import pretrain as PT, pretrain_trainer as PTT
    t = AR.MODEL_TYPE
    assert t in PTT.MODEL_TYPES and PT.ADAPT_MODEL_HEADS == {t: ("bf", "ws")}
    cls = PTT.Trainer.get_model_class(t)
    assert cls.MODEL_TYPE == t and cls.ADAPT and not cls.NOC and cls.WS_DICT_FILE == "wordset_dict5.pkl"
    assert PT.report_keys(PT.ADAPT_MODEL_HEADS[t]) == AR.report_keys() == PT.report_keys() and len(AR.report_keys()) == 13
    for ln_shared in (True, False):
        got = PT.variable_shapes(20, 7, 12, 8, 10, 6, ln_shared, ("bf", "ws"), adapt=True)
        assert got == AR.variable_shapes(20, 7, 12, 8, 10, 6, ln_shared)
        assert got["v_adapt/fc/weights"] == (10, 6) and got["pooled_linear_l/fc/weights"] == (6, 6)
        slots = sorted(k for k in got if k.startswith("v_adapt/LayerNorm") and k.endswith("/gamma"))
        assert slots == (["v_adapt/LayerNorm/gamma"] if ln_shared else ["v_adapt/LayerNorm/gamma", "v_adapt/LayerNorm_1/gamma"])
        assert PT.ln_shared_in(got) == ln_shared
        rng = np.random.default_rng(0)
        p = PT.init_random_params(rng, 20, 7, 12, 8, 10, 6, ln_shared, ("bf", "ws"), adapt=True)
        assert {k: v.shape for k, v in p.items()} == got and (p["v_adapt/LayerNorm/gamma"] == 1).all()
    # every v_adapt variable is in the last phase's bucket (its gradients need the attention backward)
    assert all(k.startswith(PT.PHASE_SCOPES[2]) for k in got if k.startswith("v_adapt/"))
    with pytest.raises(ValueError):
        PTT.Trainer.get_model_class("vlmap_bf_only_withatt_sp")


def test_variables_of_the_existing_model_types_are_unchanged(repo_root):
    """names and shapes of cfg-5, the two enwiki and the three noc models, both LayerNorm readings, as recorded from the
    commit before the adapt model"""
    from vqa_transfer_externaldata_amd import pretrain as PT
    rec = json.load(open(os.path.join(repo_root, "tests", "golden", "pretrain_variable_shapes.json")))
    d = rec["dims"]
    seen = set()
    for noc, table in ((False, PT.MODEL_HEADS), (True, PT.NOC_MODEL_HEADS)):
        for t, heads in table.items():
            for ln_shared in (True, False):
                s = PT.variable_shapes(d["Vq"], d["n_ws"], d["A"], d["W"], d["D"], d["H"], ln_shared, heads,
                                       d["n_ctx"] if "ew" in heads else None, noc)
                key = "%s|%s" % (t, "shared" if ln_shared else "per_site")
                assert {k: list(v) for k, v in s.items()} == rec["shapes"][key], key
                seen.add(key)
    assert seen == set(rec["shapes"]) and len(seen) == 12
