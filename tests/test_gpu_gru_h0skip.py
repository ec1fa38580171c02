"""The zero-state promise of the weight-stationary GRU recurrence (vqa_gru_seq_fwd_ws_ex / vqa_gru_seq_bwd_ws_ex with
h0_zero, csrc/gru_ws.hip) and its switch in the fusion step (vqa_gru_h0skip_set_mode, csrc/fusion_model.hip).

With hs[0] = 0 step 0 of the recurrence multiplies by nothing, so the flagged calls run it without matrix streams, and
the two recurrent weight-gradient GEMMs of the step skip the B tape rows of t = 0.  Held here:
  * forward and backward against the float64 reference of tests/gru_ref.py (its inputs, comparators and bounds), and
    torch.equal -- which takes -0 for +0, the one difference the skip can make -- against the general entry points on the
    same inputs with a cleared hs[0];
  * two flagged calls in a row on one workspace leave its error words clear;
  * a FusionEngine step under mode 0 and mode 3 (the default, 1, is mode 3 without the row skip): every tensor and
    gradient equal, bar the two recurrent weight blocks, whose summation is split elsewhere; those are held to the float64 product of the step's own tapes under the
    criterion of tests/gemm_ref.py for TN products, and are exactly zero at T = 1 (K = 0).
Outputs start NaN-poisoned."""
import pytest
import torch

from tests import gemm_ref
from tests import gru_ref as G
from tests.test_gpu_gru_f64 import NAN, P, _check_ws_words, _lib, _require, _ws_buffer

pytestmark = pytest.mark.gpu

H = 1024
# one half-chain, a partial chain, both sides of the switch between chains of 32 and of 64 rows (plain-order kernel /
# tails inside the streams), full chains
FWD_B = [1, 33, 256, 257, 512]
BWD_B = [257, 449, 512]
TS = [1, 2, 3]
TAPE = ("hs", "r", "u", "c", "rh")


def _inputs(T, B):
    c = G.make_inputs(T, B, H, seed=T * 7919 + B * 31 + 5, lens="random", h0="zero", device="cuda")
    assert not bool(c["h0"].any())
    return c


def _where(a, b):
    bad = (a != b).nonzero()
    return "%d elements, first at (t, row, column) = %s, worst |difference| %.3e" % (
        len(bad), tuple(int(i) for i in bad[0]), float((a - b).abs().max()))


def _forward(c, h0_zero, ws):
    L, lib = _lib()
    T, B = c["xp"].shape[:2]
    xp0 = c["xp"].clone()
    hs = torch.full((T + 1, B, H), NAN, device="cuda")
    hs[0] = 0.0                                     # the caller's part of the promise
    o = {k: torch.full((T, B, H), NAN, device="cuda") for k in ("r", "u", "c", "rh")}
    L.check(lib.vqa_gru_seq_fwd_ws_ex(P(c["xp"]), P(c["Wg"]), P(c["Wc"]), P(c["lens"]), P(hs), P(o["r"]), P(o["u"]), P(o["c"]),
                                      P(o["rh"]), T, B, H, h0_zero, P(ws), None), "vqa_gru_seq_fwd_ws_ex")
    torch.cuda.synchronize()
    _check_ws_words(ws)
    G.check_bits_unchanged(c["xp"], xp0, "xp (read only)")
    return dict(o, hs=hs)


def _backward(c, tape, outs, h0_zero, ws):
    L, lib = _lib()
    T, B = c["xp"].shape[:2]
    dxp = torch.full((T, B, 3 * H), NAN, device="cuda")
    dh = c["dh_T"].clone()
    L.check(lib.vqa_gru_seq_bwd_ws_ex(P(dh), P(c["d_outs"]) if outs else None, P(c["Wg"]), P(c["Wc"]), P(c["lens"]),
                                      P(tape["hs"]), P(tape["r"]), P(tape["u"]), P(tape["c"]), P(dxp), T, B, H, h0_zero, P(ws),
                                      None), "vqa_gru_seq_bwd_ws_ex")
    torch.cuda.synchronize()
    _check_ws_words(ws)
    G.check_bits_unchanged(dh, c["dh_T"], "dh_T (read only)")
    return dxp


@pytest.mark.parametrize("T,B", [(T, B) for T in TS for B in FWD_B])
def test_flagged_forward_matches_f64_and_the_general_call(T, B):
    _, lib = _lib()
    _require(lib.vqa_gru_ws_supported(T, B, H), "vqa_gru_seq_fwd_ws_ex")
    c = _inputs(T, B)
    ref = G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"])
    ws = _ws_buffer(T)
    got = _forward(c, 1, ws)
    worst = G.check_forward(got, ref, c["lens"])
    print("H0SKIP fwd T %d B %3d  worst %.2e (bound %.0e)" % (T, B, max(worst.values()), G.FWD_ATOL))
    general = _forward(c, 0, ws)
    G.check_forward(general, ref, c["lens"])
    for k in TAPE:
        assert torch.equal(got[k], general[k]), "%s differs from vqa_gru_seq_fwd_ws on a cleared hs[0]: %s" % (k, _where(got[k], general[k]))


@pytest.mark.parametrize("T,B,outs", [(T, B, o) for T in TS for B in BWD_B for o in (False, True)])
def test_flagged_backward_matches_f64_and_the_general_call(T, B, outs):
    _, lib = _lib()
    _require(lib.vqa_gru_ws_bwd_supported(T, B, H), "vqa_gru_seq_bwd_ws_ex")
    c = _inputs(T, B)
    tape = {k: v.float() for k, v in G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"]).items()}
    ref = G.backward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], c["dh_T"], c["d_outs"] if outs else None)
    ws = _ws_buffer(T)
    dxp = _backward(c, tape, outs, 1, ws)
    worst = G.check_backward(dxp, ref, c["lens"])
    print("H0SKIP bwd T %d B %3d outs %d  worst %.2e (bound %.0e)" % (T, B, outs, worst, G.BWD_RTOL))
    general = _backward(c, tape, outs, 0, ws)
    G.check_backward(general, ref, c["lens"])
    assert torch.equal(dxp, general), "dxp differs from vqa_gru_seq_bwd_ws: %s" % _where(dxp, general)


def test_consecutive_flagged_calls_on_one_workspace():
    """a flagged forward, then a flagged backward on its tape, on one workspace: right both times, error words clear"""
    _, lib = _lib()
    T, B = 3, 449
    _require(lib.vqa_gru_ws_bwd_supported(T, B, H), "vqa_gru_seq_bwd_ws_ex")
    c = _inputs(T, B)
    ws = _ws_buffer(T)
    tape = _forward(c, 1, ws)
    G.check_forward(tape, G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"]), c["lens"])
    ref = G.backward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], c["dh_T"], c["d_outs"])
    G.check_backward(_backward(c, tape, True, 1, ws), ref, c["lens"])
    _check_ws_words(ws)


# every intermediate of a vlmap_answer step that the forward or the backward writes (scratch of the GEMMs, of the
# reductions and of the recurrence's hand-offs is not state)
STEP_TENSORS = ("V_ft", "pre_v", "v_linear_v", "x_tm", "xp", "hs", "gru_r", "gru_u", "gru_c", "gru_rh", "pre_qv", "q_linear_v",
                "att_score", "pooled_V_ft", "pooled_linear_l", "l_linear_l", "joint_in", "joint", "logit", "pred", "report",
                "dlogit", "d_joint", "d_pre_j", "d_joint_in", "d_pl", "d_ll", "d_pooled", "d_v", "d_pre_v", "d_qv", "d_pre_qv",
                "dxp", "dx_embed", "dwx_cat")


@pytest.mark.parametrize("T", [1, 3])
def test_engine_step_mode_3_against_mode_0(T):
    """vqa_gru_h0skip_set_mode: B = 257 puts the step on the weight-stationary forward and backward; every other size is
    the smallest multiple of 4, which keeps each GEMM operand on 16-byte rows"""
    from tests.gpu_util import make_case, make_engine
    from tests.test_gpu_fusion import run_engine
    _, lib = _lib()
    B, R, N = 257, 4, 4
    dims = dict(Vq=4, W=4, D=4, H=H, A=4)
    _require(lib.vqa_gru_ws_bwd_supported(T, B, H), "vqa_gru_seq_bwd_ws_ex")
    # (the oracle's ragged questions are at least 3 tokens long: at T = 1 every question has its one token)
    p, table, nbox, batch, am, masks = make_case(1400 + T, "vlmap_answer", B, R, T, N, dims, ragged=T >= 3)
    default = lib.vqa_gru_h0skip_set_mode(-1)
    assert default == 1                             # the kernels' part; the dWh row skip (bit 1) is opt-in
    runs = {}
    try:
        for mode in (0, 3):
            assert lib.vqa_gru_h0skip_set_mode(mode) == mode
            eng = make_engine("vlmap_answer", p, table, nbox, am, B, R, T, dims, deterministic=True)
            run_engine(eng, batch, masks)
            eng.check_recurrence()
            runs[mode] = dict(grads={n: eng.grads[n].clone() for n in eng.train_names},
                              **{k: eng.tensor(k).clone() for k in STEP_TENSORS})
    finally:
        lib.vqa_gru_h0skip_set_mode(-1)
    a, b = runs[0], runs[3]
    for k in STEP_TENSORS:
        assert torch.equal(a[k], b[k]), "%s differs between the modes" % k
    wg = next(n for n in a["grads"] if n.endswith("gates/kernel"))
    wc = next(n for n in a["grads"] if n.endswith("candidate/kernel"))
    W = dims["W"]
    for n in a["grads"]:
        ga, gb = a["grads"][n], b["grads"][n]
        if n in (wg, wc):                           # the x rows come from another GEMM
            ga, gb = ga[:W], gb[:W]
        assert torch.equal(ga, gb), "%s differs between the modes" % n
    # the two recurrent blocks against the float64 product of the step's own tapes
    hs = b["hs"].view(T + 1, B, H)[:-1].reshape(T * B, H).double()
    rh = b["gru_rh"].view(T * B, H).double()
    dxp = b["dxp"].view(T * B, 3 * H).double()
    assert not bool(hs[:B].any()) and not bool(rh[:B].any())       # the rows the skip leaves out
    for name, tape, d in ((wg, hs, dxp[:, :2 * H]), (wc, rh, dxp[:, 2 * H:])):
        r64, scale = (tape.t() @ d).cpu().numpy(), (tape.abs().t() @ d.abs()).cpu().numpy()
        for mode, run in runs.items():
            got = run["grads"][name][W:].cpu().numpy()
            if T == 1:
                assert not got.any(), "%s, mode %d: the recurrent block is not zero at T = 1" % (name, mode)
            frac = gemm_ref.compare(got, r64, scale, "real", T * B, 16, "%s recurrent block, mode %d" % (name, mode))
            print("H0SKIP step T %d %s mode %d: worst error %.3f of the bound" % (T, name.split("/")[-2], mode, frac))
