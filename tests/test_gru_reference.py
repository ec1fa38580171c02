"""The float64 GRU reference (tests/gru_ref.py) that the GPU op tests of the recurrence are judged against: it
reproduces the NumPy oracle's encode_L (forward state, and through the input projection the GRU and embedding
gradients of its hand-written BPTT), and its comparator, at the tolerances the GPU tests use, rejects each of the
localized mistakes a kernel of the recurrence could make while a float32 evaluation of the contract passes."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as TR
from oracle import vqa_oracle as O
from tests import gru_ref as G

DIMS = dict(Vq=30, W=12, D=24, H=16, A=21)


def test_reference_reproduces_the_oracle_state_and_gradients():
    """h0 = 0 and xp = x W_x + b: the reference's h_T is the oracle's encode_L state to 1e-12, and its dxp pushed
    through the input projection gives the oracle's GRU kernel / bias gradients and embedding slices (dL/dh_T taken
    from torch autograd of oracle/torch_ref.py, an independently composed model)."""
    rng = np.random.default_rng(5)
    B, R, T, N = 6, 6, 7, 9
    p = O.perturb_ln_params(O.init_params(rng, "vlmap_answer", dtype=np.float64, **DIMS), rng)
    table, nbox = O.make_table(rng, N, R, DIMS["D"], np.float64)
    batch = O.make_batch(rng, B, T, DIMS["Vq"], DIMS["A"], N, np.float64)
    batch["q_intseq_len"][0], batch["q_intseq_len"][1] = T, 0       # both ends of the length range
    am = O.make_answer_masks(rng, DIMS["A"], 15, np.float64, exist_all=False)
    masks = O.make_dropout_masks(rng, B, R, DIMS["H"], np.float64, model_type="vlmap_answer")
    sc = O.scope_names("vlmap_answer")
    W, H = DIMS["W"], DIMS["H"]
    Wg, bg = p[sc["gru_gates"] + "/kernel"], p[sc["gru_gates"] + "/bias"]
    Wc, bc = p[sc["gru_cand"] + "/kernel"], p[sc["gru_cand"] + "/bias"]
    lens = torch.from_numpy(batch["q_intseq_len"].astype(np.int32))

    x = torch.from_numpy(p[sc["embed"]][batch["q_intseq"]]).transpose(0, 1)        # [T,B,W] time-major
    Wx = torch.from_numpy(np.concatenate([Wg[:W], Wc[:W]], axis=1))
    xp = x @ Wx + torch.from_numpy(np.concatenate([bg, bc]))
    Wg_h, Wc_h = torch.from_numpy(Wg[W:]), torch.from_numpy(Wc[W:])
    h0 = torch.zeros(B, H, dtype=torch.float64)
    ref = G.forward(xp, Wg_h, Wc_h, lens, h0)
    h_oracle, _ = O.gru_forward(p[sc["embed"]][batch["q_intseq"]], batch["q_intseq_len"], Wg, bg, Wc, bc)
    np.testing.assert_allclose(ref["hs"][-1].numpy(), h_oracle, rtol=0, atol=1e-12)

    P = TR.params_to_torch(p, torch.float64)
    loss, mid = TR.forward(P, batch, table, nbox, am, masks, "vlmap_answer", torch.float64)
    mid["condition"].retain_grad()
    loss.backward()
    dh_T = mid["condition"].grad
    dxp = G.backward(xp, Wg_h, Wc_h, lens, h0, dh_T)

    _, _, _, _, tape = O.forward(p, batch, table, nbox, am, masks, "vlmap_answer")
    grads, dx = O.backward(p, batch, am, masks, tape, "vlmap_answer")
    dg, dc = dxp[..., :2 * H], dxp[..., 2 * H:]
    dx_ref = dg @ torch.from_numpy(Wg[:W]).T + dc @ torch.from_numpy(Wc[:W]).T
    hs, rh = ref["hs"][:-1], ref["rh"]
    got = {
        "dx": dx_ref.transpose(0, 1),
        sc["gru_gates"] + "/kernel": torch.cat([torch.einsum("tbw,tbn->wn", x, dg), torch.einsum("tbh,tbn->hn", hs, dg)]),
        sc["gru_gates"] + "/bias": dg.sum(dim=(0, 1)),
        sc["gru_cand"] + "/kernel": torch.cat([torch.einsum("tbw,tbn->wn", x, dc), torch.einsum("tbh,tbn->hn", rh, dc)]),
        sc["gru_cand"] + "/bias": dc.sum(dim=(0, 1)),
    }
    dE = torch.zeros(p[sc["embed"]].shape, dtype=torch.float64)
    dE.index_add_(0, torch.from_numpy(batch["q_intseq"].reshape(-1).astype(np.int64)), got["dx"].reshape(-1, W))
    got[sc["embed"]] = dE
    want = dict(grads, dx=dx)
    for k, v in got.items():
        w = want[k]
        assert np.abs(w).max() > 0, k
        np.testing.assert_allclose(v.numpy(), w, rtol=0, atol=1e-10 * np.abs(w).max(), err_msg=k)


# --------------------------------------------------------------------------- the comparator's teeth
T_M, B_M, H_M = 6, 9, 64


def _mut_case():
    c = G.make_inputs(T_M, B_M, H_M, seed=3)
    c["lens"][2], c["lens"][3] = 3, 1
    return c


def _run(c, lens=None, h0=None, step=G.cell, d_outs="given"):
    lens = c["lens"] if lens is None else lens
    h0 = c["h0"] if h0 is None else h0
    fwd = G.forward(c["xp"], c["Wg"], c["Wc"], lens, h0, step=step)
    fwd["hs"][0] = c["h0"].double()                  # a kernel is handed hs[0]; only what it computes can be wrong
    d = c["d_outs"] if d_outs == "given" else d_outs
    return fwd, G.backward(c["xp"], c["Wg"], c["Wc"], lens, h0, c["dh_T"], d, step=step)


def _slab_without_r(xp_t, h, Wg, Wc):
    r, u, c, rh, hn = G.cell(xp_t, h, Wg, Wc)
    H = h.shape[1]
    rh = torch.cat([rh[:, :32], h[:, 32:64], rh[:, 64:]], dim=1)        # h instead of r*h in columns 32..63
    c = torch.tanh(xp_t[:, 2 * H:] + rh @ Wc)
    return r, u, c, rh, u * h + (1 - u) * c


def _r_u_swapped(xp_t, h, Wg, Wc):
    H = h.shape[1]
    g = torch.sigmoid(xp_t[:, :2 * H] + h @ Wg)
    u, r = g[:, :H], g[:, H:]
    rh = r * h
    c = torch.tanh(xp_t[:, 2 * H:] + rh @ Wc)
    return r, u, c, rh, u * h + (1 - u) * c


def _mutations(c):
    lens_long = c["lens"].clone()
    lens_long[2] += 1                                     # 3 -> 4 (< T)
    h0_swapped = c["h0"].clone()
    h0_swapped[[4, 5]] = c["h0"][[5, 4]]
    late = torch.zeros_like(c["d_outs"])
    late[:-1] = c["d_outs"][1:]                           # d_outs_t joins at step t - 1 (the gradient wrt h_t)
    return {
        "length_off_by_one": _run(c, lens=lens_long),
        "h_instead_of_rh_in_one_slab": _run(c, step=_slab_without_r),
        "r_and_u_swapped": _run(c, step=_r_u_swapped),
        "two_rows_h0_swapped": _run(c, h0=h0_swapped),
        "one_step_of_dxp_zeroed": "zero",
        "d_outs_joined_one_step_late": _run(c, d_outs=late),
    }


@pytest.mark.parametrize("mutation", ["length_off_by_one", "h_instead_of_rh_in_one_slab", "r_and_u_swapped",
                                      "two_rows_h0_swapped", "one_step_of_dxp_zeroed", "d_outs_joined_one_step_late"])
def test_comparator_rejects_a_wrong_recurrence(mutation):
    """At H = 64 each mutated reference fails the comparator at the GPU tests' bounds (FWD_ATOL elementwise,
    BWD_RTOL per step): the bounds are tight enough to see one wrong row, one wrong 32-column slab, one wrong step."""
    c = _mut_case()
    ref, ref_dxp = _run(c)
    G.check_forward(ref, ref, c["lens"])
    G.check_backward(ref_dxp, ref_dxp, c["lens"])
    m = _mutations(c)[mutation]
    if m == "zero":
        fwd, dxp = ref, ref_dxp.clone()
        dxp[1] = 0.0                                      # an early step: gradients are smallest there
    else:
        fwd, dxp = m
    failures = []
    for check, args in ((G.check_forward, (fwd, ref, c["lens"])), (G.check_backward, (dxp, ref_dxp, c["lens"]))):
        try:
            check(*args)
        except AssertionError as e:
            failures.append(str(e))
    assert failures, mutation + " passed the comparator"
    if mutation in ("one_step_of_dxp_zeroed", "d_outs_joined_one_step_late"):
        with pytest.raises(AssertionError):
            G.check_backward(dxp, ref_dxp, c["lens"])


@pytest.mark.parametrize("H", [64, 1024])
def test_float32_evaluation_of_the_contract_passes_the_comparator(H):
    """The bounds are not tighter than float32 arithmetic allows: the reference evaluated in float32 on the CPU passes
    at T = 14 (saturating pre-activations included)."""
    c = G.make_inputs(14, 8, H, seed=9, saturate=True)
    ref = G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"])
    f32 = G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], dtype=torch.float32)
    G.check_forward(f32, ref, c["lens"])
    for d in (None, c["d_outs"]):
        ref_dxp = G.backward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], c["dh_T"], d)
        dxp = G.backward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], c["dh_T"], d, dtype=torch.float32)
        G.check_backward(dxp, ref_dxp, c["lens"])


def test_comparator_checks_the_contract_past_the_length():
    """unwritten (NaN) outputs, a state not carried bit for bit, non-zero dxp past the length, a live-form r*h that is
    not zero -- and the live form's r, u, c past the length are exempt"""
    c = G.make_inputs(5, 6, 64, seed=4)
    ref = G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"])
    ref_dxp = G.backward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], c["dh_T"])
    past = G.past_mask(c["lens"], 5)
    b = int(c["lens"].argmin())                          # a row of length 0
    assert bool(past[:, b].all())

    def bad(**kw):
        return {k: kw.get(k, v).clone() for k, v in ref.items()}

    unwritten = bad()
    unwritten["u"][4, 3, 7] = float("nan")
    not_carried = bad()
    not_carried["hs"][3, b] += 1e-12                    # within the bound, but not the carried bits
    with pytest.raises(AssertionError, match="not written"):
        G.check_forward(unwritten, ref, c["lens"])
    with pytest.raises(AssertionError, match="carried"):
        G.check_forward(not_carried, ref, c["lens"])
    leak = ref_dxp.clone()
    leak[2, b, 0] = 1e-30
    with pytest.raises(AssertionError, match="exactly 0"):
        G.check_backward(leak, ref_dxp, c["lens"])

    live = bad()
    live["rh"][past] = 0.0
    for k in ("r", "u", "c"):
        live[k][past] = float("nan")                     # not written by the live form
    G.check_forward(live, ref, c["lens"], tape_past="live")
    with pytest.raises(AssertionError, match="not written"):
        G.check_forward(live, ref, c["lens"])
    live["rh"][past] = ref["rh"][past]
    with pytest.raises(AssertionError, match="rh: not zero"):
        G.check_forward(live, ref, c["lens"], tape_past="live")

    poisoned = torch.full((3, 4, 8), float("nan"))
    touched = poisoned.clone()
    touched[:, 1:3] = 1.0
    G.check_bits_unchanged(touched, poisoned, "window", row0=1, rows=2)
    with pytest.raises(AssertionError, match="changed"):
        G.check_bits_unchanged(touched, poisoned, "window", row0=1, rows=1)
