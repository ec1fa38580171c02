"""The float64 row-kernel references (tests/rowop_ref.py) that the GPU op tests are judged against: they reproduce the
oracle's independent code where it exists (reverse_sequence, the legacy LSTM, LayerNorm + tanh, Adam, the
marginal-entropy regulariser's pairing and tape, the report), and the comparators, at the bounds the GPU tests use,
reject localized mistakes a kernel could make while a float32 evaluation of the same contract passes."""
import numpy as np
import pytest
import torch

from oracle import bi_oracle as BO
from oracle import legacy_vqa_oracle as LO
from oracle import vqa_oracle as O
from tests import rowop_ref as R

DIMS = dict(Vq=30, W=12, D=24, H=16, A=21)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# --------------------------------------------------------------------------------------------------- against the oracle
def test_reverse_tokens_and_bi_outputs_match_reverse_sequence():
    rng = np.random.default_rng(0)
    B, T, h = 7, 6, 5
    lens = np.array([0, 1, T, 3, 4, 2, 5], np.int32)
    q = rng.integers(0, 100, (B, T)).astype(np.int32)
    assert torch.equal(R.reverse_tokens(_t(q), _t(lens)), _t(BO.reverse_sequence(q, lens)))
    # lengths past T and below 0 are clamped
    wild = np.array([T + 3, -1, T, 0, 1, 2, 3], np.int32)
    assert torch.equal(R.reverse_tokens(_t(q), _t(wild)), _t(BO.reverse_sequence(q, np.clip(wild, 0, T))))

    # bidirectional_dynamic_rnn: the backward cell runs on the reversed inputs and its outputs are reversed back
    hs_fw, hs_bw = _t(rng.standard_normal((T + 1, B, h))), _t(rng.standard_normal((T + 1, B, h)))
    q_map, q_ft = R.bi_outputs_fwd(hs_fw, hs_bw, _t(lens))
    out_bw = hs_bw[1:].permute(1, 0, 2).numpy() * (np.arange(T)[None, :, None] < lens[:, None, None])
    np.testing.assert_array_equal(q_map[:, :, h:].numpy(), BO.reverse_sequence(out_bw, lens))
    out_fw = hs_fw[1:].permute(1, 0, 2).numpy() * (np.arange(T)[None, :, None] < lens[:, None, None])
    np.testing.assert_array_equal(q_map[:, :, :h].numpy(), out_fw)
    np.testing.assert_array_equal(q_ft.numpy(), np.concatenate([hs_fw[T], hs_bw[T]], 1))


def test_lstm_step_reproduces_the_legacy_oracle():
    rng = np.random.default_rng(1)
    N, T, W, L = 6, 5, 7, 4
    x = rng.standard_normal((N, T, W))
    K, b = rng.standard_normal((W + L, 4 * L)) * 0.5, rng.standard_normal(4 * L) * 0.5
    lens = np.array([0, 1, T, 3, 2, 4], np.int32)
    c, h = torch.zeros(N, L, dtype=torch.float64), torch.zeros(N, L, dtype=torch.float64)
    for t in range(T):
        pre = torch.cat([_t(x[:, t]), h], 1) @ _t(K) + _t(b)
        _, c, h = R.lstm_step_fwd(pre, c, h, _t(lens), t)
    np.testing.assert_allclose(h.numpy(), LO.lstm_final_h(x, lens, K, b), rtol=0, atol=1e-14)


def test_ln_act_matches_the_oracle_layer_norm():
    rng = np.random.default_rng(2)
    G, rows, N = 3, 4, 10
    pre = rng.standard_normal((G, rows, N)) * 3 + 1
    gamma, beta = rng.standard_normal(N), rng.standard_normal(N)
    ln, _, _ = O.layer_norm_forward(pre, gamma, beta)
    for act, f in ((0, lambda v: np.maximum(v, 0)), (1, np.tanh)):
        y, mean, rstd, _ = R.ln_act_fwd(_t(pre.reshape(G * rows, N)), _t(gamma), _t(beta), None, 1.0, G, rows, act)
        np.testing.assert_allclose(y.numpy().reshape(G, rows, N), f(ln), rtol=0, atol=1e-13)
        np.testing.assert_allclose(mean.numpy(), pre.reshape(G, -1).mean(1), rtol=1e-14)
    # fc_ln_tanh_forward (the pre-training path's tanh layer), one row per group
    p = {"s/fc/weights": rng.standard_normal((5, N)), "s/fc/biases": rng.standard_normal(N),
         "s/LayerNorm/gamma": gamma, "s/LayerNorm/beta": beta}
    xin = rng.standard_normal((7, 5))
    y_or, _ = O.fc_ln_tanh_forward(xin, p, "s")
    y, _, _, _ = R.ln_act_fwd(_t(xin @ p["s/fc/weights"] + p["s/fc/biases"]), _t(gamma), _t(beta), None, 1.0, 7, 1, 1)
    np.testing.assert_allclose(y.numpy(), y_or, rtol=0, atol=1e-13)


def test_clip_adam_follows_the_oracle_over_several_steps():
    rng = np.random.default_rng(3)
    n, lr = 37, 1e-3
    params = {"w": rng.standard_normal(n)}
    state = O.new_opt_state()
    p, m, v = _t(params["w"].copy()), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 8):
        g = rng.standard_normal(n) * (10.0 if t % 2 else 0.1)          # clip active on odd steps only
        norm = O.clip_adam_step(params, {"w": g}, ["w"], state, lr, None, "embed")
        assert abs(float(R.sumsq(_t(g))) ** 0.5 - norm) <= 1e-12 * norm
        p, m, v = R.clip_adam(p, _t(g), m, v, norm, O.CLIP_NORM, R.adam_lr(lr, t))
        np.testing.assert_allclose(p.numpy(), params["w"], rtol=0, atol=1e-14)
        np.testing.assert_allclose(m.numpy(), state["m"]["w"], rtol=1e-13)
        np.testing.assert_allclose(v.numpy(), state["v"]["w"], rtol=1e-13)


def test_tile_mul_and_marginal_entropy_reproduce_the_entropy_model():
    """vlmap_answer_ent: the pairing of tile_mul is the oracle's marginal_index, and marginal_entropy on the oracle's
    pairing logits gives its probabilities, marginal and entropy"""
    rng = np.random.default_rng(4)
    B, R_, T, N, M = 5, 6, 7, 9, 3
    mt = "vlmap_answer_ent"
    p = O.perturb_ln_params(O.init_params(rng, mt, dtype=np.float64, **DIMS), rng)
    table, nbox = O.make_table(rng, N, R_, DIMS["D"], np.float64)
    batch = O.make_batch(rng, B, T, DIMS["Vq"], DIMS["A"], N, np.float64)
    am = O.make_answer_masks(rng, DIMS["A"], 15, np.float64, exist_all=False)
    masks = O.make_dropout_masks(rng, B, R_, DIMS["H"], np.float64, model_type=mt, num_marginal=M)
    _, report, _, mid, tape = O.forward(p, batch, table, nbox, am, masks, mt)
    te, sc = tape["t_ent"], O.scope_names(mt)

    pl, ll = _t(tape["pl"]), _t(tape["ll"])
    tin = R.tile_mul_fwd(pl, ll, M).view(B, M, -1)
    np.testing.assert_array_equal(tin.numpy(), te["tp"] * tape["ll"][:, None, :])
    assert torch.equal(R.tile_src(B, M).view(B, M), _t(O.marginal_index(B, M)))

    A = DIMS["A"]
    tz = te["tj"] @ p[sc["head"] + "/fc/weights"] + p[sc["head"] + "/fc/biases"]
    prob, marg, ent, _, _ = R.marginal_entropy(_t(tz.reshape(B * M, A)), _t(am["train"]), _t(am["exist"]), 0.1 / B,
                                               B, M, A)
    sel = te["sel"]
    np.testing.assert_allclose(prob.view(B, M, A).numpy()[:, :, sel], te["prob"], rtol=0, atol=1e-14)
    assert float(prob.view(B, M, A)[:, :, ~torch.from_numpy(sel)].abs().max()) == 0.0
    np.testing.assert_allclose(marg.numpy()[:, sel], te["mprob"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(float(ent.mean()), report["entropy"], rtol=1e-13)
    np.testing.assert_allclose(mid["marginal_prob"], marg.numpy()[:, sel], rtol=0, atol=1e-14)


def test_marginal_entropy_of_an_empty_selection_is_zero():
    """the header's definition, and the oracle's: the entropy of a softmax over no answers is 0"""
    tz = torch.randn(6, 9, dtype=torch.float64)
    prob, marg, ent, dz, _ = R.marginal_entropy(tz, torch.zeros(9), torch.ones(9), 0.1, 2, 3, 9)
    for t in (prob, marg, ent, dz):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0


def test_report_reduce_reproduces_the_oracle_report():
    rng = np.random.default_rng(5)
    B, A = 9, 21
    z = rng.standard_normal((B, A))
    tgt = np.zeros((B, A))
    tgt[np.arange(B), rng.integers(0, A, B)] = 1.0
    tgt[0, :] = 0.0                                                  # a question without a positive answer
    for zero_test in (False, True):
        am = O.make_answer_masks(rng, A, 15, np.float64, exist_all=False)
        if zero_test:
            am["train"][:] = 1.0                                     # no test answers: the test ratios' den is 0
        _, report, out, ell = O.loss_and_report(z, tgt, am, "vlmap_answer")
        tr, ob, at, ex = am["train"], am["obj"], am["attr"], am["exist"]
        te = 1 - tr
        pred = out["pred"]
        tp = tgt[np.arange(B), pred]
        stats = np.zeros((B, R.STAT_COUNT))
        stats[:, R.S_LOSS_TRAIN] = (ell * tr).sum(1)
        stats[:, R.S_LOSS_REPORT] = ell.sum(1)
        stats[:, R.S_ALL] = tp
        stats[:, R.S_EXIST] = tp * ex[pred]
        stats[:, R.S_TEST] = tp * te[pred]
        stats[:, R.S_TEST_OBJ] = tp * (te * ob)[pred]
        stats[:, R.S_TEST_ATTR] = tp * (te * at)[pred]
        stats[:, R.S_TRAIN_EXIST] = tp * (ex * tr)[pred]
        stats[:, R.S_MAX_EXIST] = (tgt * ex).max(1)
        stats[:, R.S_MAX_TRAIN_EXIST] = (tgt * ex * tr).max(1)
        stats[:, R.S_TEST_OBJ_MAX] = (tgt * te * ob).max(1)
        stats[:, R.S_TEST_ATTR_MAX] = (tgt * te * at).max(1)
        stats[:, R.S_TEST_MAX] = (tgt * te).max(1)
        stats[:, R.S_TEST_MAX_EXIST] = (tgt * ex * te).max(1)
        rep, _ = R.report_reduce(_t(stats))
        np.testing.assert_allclose(rep.numpy(), [report[k] for k in O.REPORT_KEYS], rtol=1e-13, atol=0)


def test_backward_references_are_autograd_of_their_forwards():
    """spot checks against central differences (the references are autograd; this guards the loss each one states)"""
    torch.manual_seed(6)
    eps = 1e-6
    mean, ls, noise, dx = (torch.randn(2, 5, dtype=torch.float64) for _ in range(4))
    dm, dl = R.reparam_bwd(dx, mean, ls, noise, 0.3)
    loss = lambda m, l: float((dx * R.reparam_fwd(m, l, noise)[0]).sum() + 0.3 * R.reparam_fwd(m, l, noise)[1].sum())
    e = torch.zeros_like(ls)
    e[1, 2] = eps
    assert abs((loss(mean, ls + e) - loss(mean, ls - e)) / (2 * eps) - float(dl[1, 2])) < 1e-7
    # the header's closed forms
    torch.testing.assert_close(dm, dx + 0.3 * mean)
    torch.testing.assert_close(dl, dx * noise * torch.exp(ls).sqrt() / 2 + 0.3 * (torch.exp(ls) - 1) / 2)


# ------------------------------------------------------------------------------------------------------ the comparators
def test_index_comparator_rejects_an_off_by_one_bw_row():
    """one row of q_map's backward half taken from hs_bw[len - t - 1] instead of hs_bw[len - t]"""
    torch.manual_seed(7)
    B, T, h = 5, 6, 4
    lens = torch.tensor([6, 3, 0, 1, 4], dtype=torch.int32)
    hs_fw, hs_bw = torch.randn(T + 1, B, h), torch.randn(T + 1, B, h)
    q_map, q_ft = R.bi_outputs_fwd(hs_fw, hs_bw, lens)
    R.check_bits(q_map, R.bi_outputs_fwd(hs_fw.double(), hs_bw.double(), lens)[0], "float32 copy")
    bad = q_map.clone()
    b, n = 1, 3
    for t in range(n):
        bad[b, t, h:] = hs_bw[n - t - 1, b]
    with pytest.raises(AssertionError, match="differ"):
        R.check_bits(bad, q_map.double(), "q_map")


def _marginal_f32_and_ref(cols=1000, B=3, M=5):
    g = torch.Generator().manual_seed(8)
    tz = torch.randn(B * M, cols, generator=g) * 3
    train = (torch.rand(cols, generator=g) < 0.8).float()
    exist = torch.ones(cols)
    ref = R.marginal_entropy(tz, train, exist, 0.1 / B, B, M, cols)
    f32 = R.marginal_entropy(tz, train, exist, 0.1 / B, B, M, cols, dtype=torch.float32)
    return tz, train, exist, ref, f32


def _check_marginal(got, ref):
    prob, marg, ent, dz, escale = ref
    R.check_elementwise(got[0], prob, "prob")
    R.check_elementwise(got[1], marg, "marginal")
    R.check_rows(got[2], ent, "ent_row", scale=escale + marg.sum(1), rtol=R.RTOL["marginal_entropy ent_row"])
    R.check_rows(got[3], dz, "dz", rtol=R.RTOL["marginal_entropy dz"])


def test_marginal_comparator_rejects_one_wrong_256_column_block():
    """one 256-column block of one question's marginal averaged over M - 1 of its M pairings"""
    tz, train, exist, ref, f32 = _marginal_f32_and_ref()
    _check_marginal(f32, ref)
    B, M = 3, 5

    def tamper(prob, marg):
        out = marg.clone()
        out[1, 256:512] = prob.view(B, M, -1)[1, :M - 1, 256:512].mean(0)
        return out
    bad = R.marginal_entropy(tz, train, exist, 0.1 / B, B, M, 1000, dtype=torch.float32, tamper=tamper)
    with pytest.raises(AssertionError, match="marginal"):
        _check_marginal(bad, ref)
    with pytest.raises(AssertionError, match="dz"):
        R.check_rows(bad[3], ref[3], "dz", rtol=R.RTOL["marginal_entropy dz"])


def test_adam_comparator_rejects_a_wrong_tail_element():
    """the last element (the float4 body's tail, block 0's work) updated with the unclipped gradient"""
    g = torch.Generator().manual_seed(9)
    n = 4097
    p, m, v = torch.randn(n, generator=g) * 0.01, torch.zeros(n), torch.zeros(n)
    rp, rm, rv = p.double(), m.double(), v.double()
    fp, fm, fv = p, m, v
    bp, bm, bv = p, m, v
    for t in range(1, 4):
        gr = torch.randn(n, generator=g)
        gr[-1] = 1.0
        norm = float(R.sumsq(gr)) ** 0.5
        clip, lr_t = 0.5 * norm, R.adam_lr(1e-2, t)
        rp, rm, rv = R.clip_adam(rp, gr, rm, rv, norm, clip, lr_t)
        fp, fm, fv = R.clip_adam(fp, gr, fm, fv, norm, clip, lr_t, dtype=torch.float32)
        bp, bm, bv = R.clip_adam(bp, gr, bm, bv, norm, clip, lr_t, dtype=torch.float32, tail=(n - 1, 1.0))
        blocks = lambda x: torch.cat([x, x.new_zeros((-n) % 1024)]).view(-1, 1024)
        for name, a, r in (("p", fp, rp), ("m", fm, rm), ("v", fv, rv)):
            R.check_rows(blocks(a), blocks(r), name, rtol=R.RTOL["clip_adam " + name])
        # m / sqrt(v) does not see a per-element gradient scale, so p cannot show this mistake; m and v do
        for name, a, r in (("m", bm, rm), ("v", bv, rv)):
            with pytest.raises(AssertionError, match="row 4 "):
                R.check_rows(blocks(a), blocks(r), name, rtol=R.RTOL["clip_adam " + name])


def test_tile_comparator_rejects_one_row_paired_by_row_mod_M():
    torch.manual_seed(10)
    B, M, H = 5, 3, 301
    pl, ll = torch.randn(B, H), torch.randn(B, H)
    ref = R.tile_mul_fwd(pl, ll, M)
    R.check_bits(R.tile_mul_fwd(pl, ll, M, dtype=torch.float32), ref, "float32 product")
    src = R.tile_src(B, M).clone()
    src[7] = 7 % M                                               # (7 % B = 2) != (7 % M = 1)
    with pytest.raises(AssertionError, match="differ"):
        R.check_bits(R.tile_mul_fwd(pl, ll, M, dtype=torch.float32, src=src), ref, "tile_mul_fwd")
    dx = torch.randn(B * M, H)
    R.check_rows(R.tile_mul_bwd(dx, pl, ll, M, dtype=torch.float32), R.tile_mul_bwd(dx, pl, ll, M), "dll",
                 rtol=R.RTOL["tile_mul_bwd"])


def test_lstm_comparator_rejects_a_dropped_forget_bias_on_one_column():
    torch.manual_seed(11)
    N, L, t = 9, 65, 2
    pre, c, h = torch.randn(N, 4 * L), torch.randn(N, L), torch.randn(N, L) * 0.5
    lens = torch.tensor([0, 2, 3, 5, 9, 1, 3, 4, 6], dtype=torch.int32)
    ref = R.lstm_step_fwd(pre, c, h, lens, t)
    got = R.lstm_step_fwd(pre, c, h, lens, t, dtype=torch.float32)
    R.check_rows(got[0], ref[0], "gates", rtol=0.0, atol=R.ABS_BOUNDED)
    R.check_rows(got[1], ref[1], "c_new", rtol=R.RTOL["lstm_step_fwd c_new"])
    R.check_rows(got[2], ref[2], "h_new", rtol=0.0, atol=R.ABS_BOUNDED)

    def cell(g, c_prev):
        act, cn, hn = R.lstm_cell(g, c_prev)
        act2, cn2, hn2 = R.lstm_cell(g, c_prev, forget_bias=0.0)
        k = 17
        act[:, 2 * L + k], cn[:, k], hn[:, k] = act2[:, 2 * L + k], cn2[:, k], hn2[:, k]
        return act, cn, hn
    bad = R.lstm_step_fwd(pre, c, h, lens, t, dtype=torch.float32, cell=cell)
    with pytest.raises(AssertionError, match="gates"):
        R.check_rows(bad[0], ref[0], "gates", rtol=0.0, atol=R.ABS_BOUNDED)
    with pytest.raises(AssertionError, match="c_new"):
        R.check_rows(bad[1], ref[1], "c_new", rtol=R.RTOL["lstm_step_fwd c_new"])
    # the backward of a float32 evaluation also passes
    dh, dc = torch.randn(N, L), torch.randn(N, L)
    for name, a, r in zip(("dgates", "dc_prev", "dh_carry"), R.lstm_step_bwd(dh, dc, pre, c, h, lens, t, torch.float32),
                          R.lstm_step_bwd(dh, dc, pre, c, h, lens, t)):
        R.check_rows(a, r, name, rtol=R.RTOL.get("lstm_step_bwd " + name, 0.0))


def test_float32_evaluations_pass_the_remaining_comparators():
    torch.manual_seed(12)
    f = torch.float32
    # reparameterisation
    mean, noise, dx = torch.randn(3, 300), torch.randn(3, 300), torch.randn(3, 300)
    ls = torch.linspace(-15, 15, 900).view(3, 300)
    rx, rkl, sc = R.reparam_fwd(mean, ls, noise)
    x, kl, _ = R.reparam_fwd(mean, ls, noise, f)
    R.check_rows(x, rx, "x", rtol=R.RTOL["reparam_fwd x"])
    R.check_rows(kl, rkl, "kl_row", scale=sc, rtol=R.RTOL["reparam_fwd kl_row"])
    for a, r in zip(R.reparam_bwd(dx, mean, ls, noise, 0.01, f), R.reparam_bwd(dx, mean, ls, noise, 0.01)):
        R.check_rows(a, r, "reparam_bwd", rtol=R.RTOL["reparam_bwd dmean"])
    # scoring layer
    al, pq, w, b = torch.randn(257, 65) * 0.7, torch.randn(4, 65) * 0.7, torch.randn(65) / 8, torch.tensor([0.3])
    R.check_rows(R.score_fwd(al, pq, w, b, f), R.score_fwd(al, pq, w, b), "z", rtol=R.RTOL["score_fwd"])
    dz = torch.randn(4, 257) / 257
    for name, a, r in zip(("d_al", "d_pq", "part_dw"), R.score_bwd(dz, al, pq, w, b, f), R.score_bwd(dz, al, pq, w, b)):
        R.check_rows(a, r, name, rtol=R.RTOL["score_bwd " + name])
    # LayerNorm + tanh, with a keep-mask
    G, rows, N = 3, 5, 300
    pre, gamma, beta = torch.randn(G * rows, N) * 2, 1 + 0.2 * torch.randn(N), 0.2 * torch.randn(N)
    keep = (torch.rand(G * rows, N) < 0.5).to(torch.uint8)
    ry = R.ln_act_fwd(pre, gamma, beta, keep, 0.5, G, rows, 1)[0]
    R.check_rows(R.ln_act_fwd(pre, gamma, beta, keep, 0.5, G, rows, 1, f)[0], ry, "y", rtol=0.0, atol=2 * R.ABS_BOUNDED)
    dy = torch.randn(G * rows, N)
    got, ref = (R.ln_act_bwd(dy, pre, gamma, beta, keep, 0.5, G, rows, 1, d) for d in (f, torch.float64))
    R.check_rows(got[0].view(G, -1), ref[0].view(G, -1), "dpre", rtol=R.RTOL["ln_act(tanh)_bwd dpre"])
    for a, r in zip(got[1:3], ref[1:3]):
        R.check_rows(a, r, "part", rtol=R.RTOL["ln_act(tanh)_bwd part_dgamma"])
    # embedding scatter
    T, B, W, Vq = 5, 40, 16, 9
    dxt, q = torch.randn(T, B, W), torch.randint(-2, Vq + 2, (B, T), dtype=torch.int32)
    lens = torch.randint(-1, T + 3, (B,), dtype=torch.int32)
    R.check_rows(R.embed_bwd_len(dxt, q, lens, Vq, f), R.embed_bwd_len(dxt, q, lens, Vq), "dE", rtol=R.RTOL["embed_bwd_len_det"])
    # report
    stats = torch.rand(1000, R.STAT_COUNT)
    ref, scale = R.report_reduce(stats)
    R.check_rows(R.report_reduce(stats, f)[0], ref, "report", scale=scale, rtol=R.RTOL["report_reduce"])
    # one GRU step and its backward
    B, H, t = 37, 300, 2
    gpre, cpre, h = torch.randn(B, 2 * H) * 2, torch.randn(B, H) * 2, torch.randn(B, H) * 0.5
    ln = torch.randint(0, 5, (B,), dtype=torch.int32)
    for name, a, r in zip("r u rh c h_new".split(), R.gru_step_fwd(gpre, cpre, h, ln, t, f),
                          R.gru_step_fwd(gpre, cpre, h, ln, t)):
        R.check_rows(a, r, name, rtol=0.0, atol=R.ABS_BOUNDED)
    dh, drh = torch.randn(B, H), torch.randn(B, H)
    for name, a, r in zip(("dr_pre", "du_pre", "dc_pre", "dh_acc"), R.gru_step_bwd(dh, drh, gpre, cpre, h, ln, t, f),
                          R.gru_step_bwd(dh, drh, gpre, cpre, h, ln, t)):
        R.check_rows(a, r, name, rtol=R.RTOL["gru_step_bwd " + name])
