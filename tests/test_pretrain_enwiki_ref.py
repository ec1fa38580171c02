"""CPU checks of the enwiki-context pre-training models' float64 reference (tests/pretrain_enwiki_ref.py) and of their
host side: model registry, variable names and LayerNorm slots, enwiki context sampling."""
import numpy as np
import pytest

from oracle import pretrain_oracle as PO
from tests import pretrain_enwiki_ref as ER

DIMS = dict(B=3, n=5, R=6, D=10, H=6, L=4, W=8, Vq=20, n_ws=7, A=12, n_ctx=15, Lc=7)


def _case(seed=0, heads=ER.HEADS_ALL, ln_shared=True, dims=DIMS):
    d = dims
    rng = np.random.default_rng(seed)
    p = ER.init_params(rng, d["Vq"], d["n_ws"], d["A"], W=d["W"], D=d["D"], H=d["H"], ln_shared=ln_shared, heads=heads,
                       n_ctx=d["n_ctx"], dtype=np.float64)
    b = PO.make_batch(rng, d["B"], d["n"], d["R"], d["D"], d["L"], d["Vq"], d["n_ws"], d["A"], dtype=np.float64)
    b = ER.add_enwiki_fields(rng, b, d["n_ctx"], d["Lc"])
    m = ER.add_enwiki_masks(rng, PO.make_masks(rng, d["B"], d["n"], d["R"], d["H"], dtype=np.float64), d["B"], d["n"],
                            d["H"], dtype=np.float64)
    return p, b, m


@pytest.mark.parametrize("ln_shared", [True, False])
def test_without_enwiki_heads_both_equal_the_cfg5_oracle(ln_shared):
    p, b, m = _case(1, heads=("bf", "ws"), ln_shared=ln_shared)
    assert sorted(p) == sorted(PO.variable_shapes(20, 7, 12, W=8, D=10, H=6, ln_shared=ln_shared))
    total, rep, mid = ER.forward(p, b, m, 5, ("bf", "ws"))
    t0, r0, mid0 = PO.forward(p, b, m, 5)
    assert abs(total - t0) <= 1e-12 * abs(t0) and sorted(rep) == sorted(r0)
    for k in r0:
        assert abs(rep[k] - r0[k]) <= 1e-12 * max(1.0, abs(r0[k])), k
    for k in PO.KINDS:
        np.testing.assert_allclose(mid[k + "/bf_logit"], mid0[k + "/bf_logit"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(mid[k + "/ws_logit"], mid0[k + "/ws_logit"], rtol=0, atol=1e-12)
    cap, cap0 = {}, {}
    tt, losses, g, sl = ER.torch_loss_and_grads(p, b, m, 5, ("bf", "ws"), capture=cap)
    tt0, losses0, g0, sl0 = PO.torch_loss_and_grads(p, b, m, 5, capture=cap0)
    assert abs(tt - tt0) <= 1e-12 * abs(tt0) and abs(tt - total) <= 1e-10 * abs(total)
    for k in g0:
        sc = max(np.abs(g0[k]).max(), 1e-30)
        assert np.abs(g[k] - g0[k]).max() <= 1e-12 * sc, k
    for k in sl0:
        np.testing.assert_allclose(sl[k], sl0[k], rtol=0, atol=1e-12 * max(np.abs(sl0[k]).max(), 1e-30))
    assert set(ER.relu_sites(("bf", "ws"))) == set(PO.RELU_SITES)
    for s in PO.RELU_SITES:
        assert np.array_equal(cap[s], cap0[s]), s
    # gate conditioning reproduces the unconditioned run when handed its own gates
    _, _, gg, _ = ER.torch_loss_and_grads(p, b, m, 5, ("bf", "ws"), gates=cap)
    for k in g:
        assert np.abs(gg[k] - g[k]).max() <= 1e-12 * max(np.abs(g[k]).max(), 1e-30), k


@pytest.mark.parametrize("heads", [("bf", "ws", "ew"), ("bf", "ew")])
def test_numpy_forward_equals_torch_and_report_keys(heads):
    p, b, m = _case(2, heads=heads, ln_shared=False)
    total, rep, mid = ER.forward(p, b, m, 5, heads)
    tt, losses, g, sl = ER.torch_loss_and_grads(p, b, m, 5, heads)
    assert abs(tt - total) <= 1e-10 * abs(total)
    assert list(rep)[-1] == "total_loss" and sorted(rep) == sorted(ER.report_keys(heads))
    assert len(rep) == (19 if "ws" in heads else 13)
    for k, v in losses.items():
        assert abs(rep[k + "_loss"] - v) <= 1e-10 * abs(v), k
    assert "obj/enwiki_embed" in sl and sl["attr/enwiki_embed"].shape == (15, 7, 8)
    if "ws" not in heads:
        assert not g["wordset_map/learn"].any() and "wordset_ft/fc/weights" not in g
    # every LayerNorm slot of the shared fusion scopes gets a gradient (head 2 r + k owns slot 2 r + k)
    for s in range(2 * len(heads)):
        assert np.abs(g[PO.ln_name("joint_fc", s) + "/gamma"]).max() > 0, s


@pytest.mark.parametrize("heads", [("bf", "ws", "ew"), ("bf", "ew")])
def test_finite_differences_on_the_enwiki_encoder_and_embedding(heads):
    p, b, m = _case(3, heads=heads, ln_shared=False)
    _, _, g, _ = ER.torch_loss_and_grads(p, b, m, 5, heads)
    rng = np.random.default_rng(4)
    used = np.unique(b["obj_blank_fill/enwiki_context"][b["obj_blank_fill/enwiki_context"] > 0])
    picks = [("enwiki_map/learn", (int(used[0]), 3)), ("enwiki_map/learn", (int(used[-1]), 0))]
    for v in ER.GRU_VARS:
        name = "encode_L_enwiki/rnn/gru_cell/" + v
        shp = p[name].shape
        picks += [(name, tuple(int(rng.integers(0, s)) for s in shp)) for _ in range(2)]
    eps = 1e-6
    for name, idx in picks:
        q = {k: v.copy() for k, v in p.items()}
        q[name][idx] += eps
        up = ER.forward(q, b, m, 5, heads)[0]
        q[name][idx] -= 2 * eps
        dn = ER.forward(q, b, m, 5, heads)[0]
        fd = (up - dn) / (2 * eps)
        assert abs(fd - g[name][idx]) <= 1e-5 * abs(fd) + 1e-9, (name, idx, fd, g[name][idx])


def test_a_localized_mutation_fails_the_gpu_bounds_and_float32_passes(monkeypatch):
    """The GPU tests' bars (report 2e-4 relative, logits 1e-3): a float32 evaluation of the reference passes them; the
    reference with the attribute enwiki head on the object head's LayerNorm slot (one head, one scope) does not."""
    heads = ER.HEADS_ALL
    dims = dict(DIMS, D=32, H=16, A=40)
    p, b, m = _case(5, heads=heads, ln_shared=False, dims=dims)
    total, rep, mid = ER.forward(p, b, m, 5, heads)
    f32 = lambda d: {k: (v.astype(np.float32) if v.dtype.kind == "f" else v) for k, v in d.items()}
    _, rep32, mid32 = ER.forward(f32(p), f32(b), f32(m), 5, heads)

    def within(r, z):
        ok = all(abs(r[k] - rep[k]) <= 2e-4 * max(1.0, abs(rep[k])) for k in rep)
        return ok and all(np.abs(z[k] - mid[k]).max() < 1e-3 for k in mid if k.endswith("_logit"))
    assert within(rep32, mid32)
    real = PO._fc_ln

    def mutated(x, q, scope, ln_idx, act):
        return real(x, q, scope, 4 if (scope == "joint_fc" and ln_idx == 5) else ln_idx, act)
    monkeypatch.setattr(PO, "_fc_ln", mutated)
    _, repm, midm = ER.forward(p, b, m, 5, heads)
    assert not within(repm, midm)
    assert np.abs(midm["obj/ew_logit"] - mid["obj/ew_logit"]).max() == 0       # localized: only that head moved


# ------------------------------------------------------------------------------------------------ host side
def test_registry_accepts_both_enwiki_models():
    from vqa_transfer_externaldata_amd import pretrain_trainer as PTT
    for mt in ("vlmap_bf_or_wordset_enwiki_withatt_sp", "vlmap_bf_enwiki_withatt_sp"):
        cls = PTT.Trainer.get_model_class(mt)
        assert cls.MODEL_TYPE == mt and mt in PTT.MODEL_TYPES
        assert PTT.build_parser().parse_args(["--model_type", mt]).model_type == mt
    assert PTT.Trainer.get_model_class().MODEL_TYPE == "vlmap_bf_or_wordset_withatt_sp"
    with pytest.raises(ValueError):
        PTT.Trainer.get_model_class("vlmap_enwiki_withatt_sp")


@pytest.mark.parametrize("ln_shared", [True, False])
@pytest.mark.parametrize("heads", [("bf", "ws", "ew"), ("bf", "ew"), ("bf", "ws")])
def test_variable_names_shapes_and_layernorm_slots(heads, ln_shared):
    from vqa_transfer_externaldata_amd import pretrain as PT
    s = PT.variable_shapes(50, 9, 40, W=300, D=2048, H=1024, ln_shared=ln_shared, heads=heads, n_ctx=77)
    assert s == ER.variable_shapes(50, 9, 40, W=300, D=2048, H=1024, ln_shared=ln_shared, heads=heads, n_ctx=77)
    if heads == ("bf", "ws"):
        assert s == PT.variable_shapes(50, 9, 40, ln_shared=ln_shared)
    last = 0 if ln_shared else 2 * len(heads) - 1
    for scope in ("pooled_linear_l", "q_linear_l", "joint_fc"):
        assert PT.ln_name(scope, last) + "/gamma" in s and PT.ln_name(scope, last + 1) + "/gamma" not in s
    if "ew" in heads:
        assert s["enwiki_map/learn"] == (77, 300) and "enwiki_map/learn" in PT.SPARSE_VARS
        assert s["encode_L_enwiki/rnn/gru_cell/gates/kernel"] == (1324, 2048)
        assert s["encode_L_enwiki/rnn/gru_cell/candidate/bias"] == (1024,)
    assert ("wordset_ft/fc/weights" in s) == ("ws" in heads) and "wordset_map/learn" in s
    assert PT.ln_shared_in(s) == ln_shared
    p = PT.init_random_params(np.random.default_rng(0), 50, 9, 40, W=8, D=16, H=8, ln_shared=ln_shared, heads=heads,
                              n_ctx=11)
    assert sorted(p) == sorted(PT.variable_shapes(50, 9, 40, W=8, D=16, H=8, ln_shared=ln_shared, heads=heads, n_ctx=11))
    assert PT.report_keys(heads) == ER.report_keys(heads)


def _ds(seed, enwiki, n_images=12):
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV
    data = DV.synthetic_dataset(n_images, 50, 9, 21, R=36, D=8, max_len=7, seed=0, enwiki=dict(n_ctx=40, Lc=7))
    return data, DV.Dataset(split="train", data=data, seed=seed, enwiki=enwiki)


def test_synthetic_enwiki_dictionary():
    data, _ = _ds(0, True)
    e = data["enwiki_dict"]
    assert e["max_context_len"] == 7 and e["np_context"].shape[1] == 7 and e["np_context"].dtype == np.int32
    lens = e["np_context_len"]
    assert lens.min() == 1 and lens.max() == 7 and set(e["ans2shuffled_context_idx"]) == set(range(21))
    assert e["context_word_vocab"][1] == "<unk>" and (e["np_context"] == 1).any()
    for row, ln in zip(e["np_context"], lens):
        assert np.all(row[:ln] > 0) and np.all(row[ln:] == 0)


def test_context_sampling_round_robin_reshuffle_and_padding():
    data, ds = _ds(3, True)
    e = data["enwiki_dict"]
    # round robin over the answer's list, reshuffled (from the context stream) when exhausted
    label = 4
    lst = e["ans2shuffled_context_idx"][label]
    lst[:] = [10, 11, 12]
    got = [ds.sample_context({"fill": label}, "obj", "fill") for _ in range(3)]
    assert got == [10, 11, 12] and ds.enwiki_choice_idx["obj"]["fill"][label] == 0
    assert sorted(lst) == [10, 11, 12]
    second = list(lst)                                               # the order after the reshuffle
    nxt = [ds.sample_context({"fill": label}, "obj", "fill") for _ in range(3)]
    assert nxt == second
    assert ds.enwiki_choice_idx["attr"]["fill"][label] == 0          # per category
    for image_id in ds.ids:
        r = ds.get_data(image_id)
        for key in ("obj_blank_fill", "attr_blank_fill"):
            c, ln = r[key + "/enwiki_context"], r[key + "/enwiki_context_len"]
            assert c.shape == (5, 7) and ln.shape == (5,) and c.dtype == np.int32 and ln.dtype == np.int32
            for j in range(5):
                hits = [i for i in e["ans2shuffled_context_idx"][int(r[key + "/fills"][j])]
                        if np.array_equal(e["np_context"][i], c[j])]
                assert hits and e["np_context_len"][hits[0]] == ln[j]
            nv = int(r[key + "/num"])
            if nv < 5:     # padding repeats the last entry: same answer, its own context draw from the same list
                assert np.all(r[key + "/fills"][nv:] == r[key + "/fills"][nv - 1])


def test_cfg5_fields_are_bit_identical_with_or_without_enwiki():
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV
    _, a = _ds(7, True)
    _, b = _ds(7, False)
    assert b.enwiki_dict is None
    ba = list(DV.create_ops(4, a, is_train=True, seed=7, repeat=2))
    bb = list(DV.create_ops(4, b, is_train=True, seed=7, repeat=2))
    assert len(ba) == len(bb) == 6
    for x, y in zip(ba, bb):
        assert sorted(set(x) - set(y)) == sorted(k + "_blank_fill/enwiki_context" + s for k in ("attr", "obj")
                                                 for s in ("", "_len"))
        for k in y:
            assert np.array_equal(x[k], y[k]), k
        assert x["obj_blank_fill/enwiki_context"].shape == (4, 5, 7)


def test_forked_producer_reseeds_the_context_stream():
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV
    _, ds = _ds(7, True)
    s0 = ds.ctx_rng.get_state()[1].copy()
    import queue as _q

    class Q:
        def __init__(self):
            self.items = []

        def put(self, x):
            self.items.append(x)
    q = Q()
    DV._worker_main(q, 4, ds, True, True, 7, 1, True, 1, 2)
    assert q.items[-1] is None and not any(isinstance(x, tuple) for x in q.items)
    assert not np.array_equal(ds.ctx_rng.get_state()[1], s0)
    del _q


def test_length_sort_covers_the_contexts():
    from vqa_transfer_externaldata_amd import pretrain as PT
    p, b, m = _case(6)
    out = PT.add_length_sort(dict(b))
    s = out["enwiki_context/sort"]
    lens = np.concatenate([b[k + "_blank_fill/enwiki_context_len"].reshape(-1) for k in PO.KINDS])
    assert np.all(np.diff(lens[s["perm"]]) <= 0) and np.array_equal(s["perm"][s["inv"]], np.arange(len(lens)))
    assert s["live_rows"].tolist() == [int((lens > t).sum()) for t in range(7)] and s["live_rows"][0] == len(lens)
    assert "blank_fill/sort" in out
