"""The reference of the bf16 GRU recurrence (tests/gru_bf16_ref.py) judged on the CPU, from the references alone: with
rounding off it is tests/gru_ref.py; on every case of the GPU op test (tests/test_gpu_gru_bf16_f64.py) the rounded and
the unrounded recurrence, and the rounded and the truncated one, sit at least 10 x the GPU test's own bound apart on hs
and on dxp -- so a kernel that ignores GRU-step id 64 (or the step's flag), or converts by truncation, cannot pass."""
import functools

import pytest
import torch

from tests import bf16_ref as R
from tests import gru_bf16_ref as Q
from tests import gru_ref as G

MARGIN = 10.0


@functools.lru_cache(maxsize=None)
def _rounded(case):
    c = Q.make_case(*case)
    ref, cell = Q.forward(c)
    dxp = {o: Q.backward(c, o)[0] for o in (False, True)}
    return c, ref, cell, dxp


def _distances(case, other_fwd, other_dxp):
    """worst |other - rounded| / (the GPU test's bound) on hs and on dxp (without and with d_outs)"""
    c, ref, cell, dxp = _rounded(case)
    fwd = Q.forward_ratio(other_fwd, ref, c["lens"], Q.forward_bounds(ref, cell))["hs"]
    bwd = min(Q.backward_ratio(other_dxp[o], dxp[o], Q.backward_bounds(c, ref, dxp[o], dxp[o])) for o in (False, True))
    return fwd, bwd


@pytest.mark.parametrize("case", Q.CASES[:6] + [Q.SATURATED])
def test_without_rounding_it_is_gru_ref(case):
    c = Q.make_case(*case)
    got, _ = Q.forward(c, rounding=False)
    want = G.forward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"])
    for k in want:
        assert float((got[k] - want[k]).abs().max()) <= 1e-12, k
    for outs in (False, True):
        dxp, _ = Q.backward(c, outs, rounding=False)
        want = G.backward(c["xp"], c["Wg"], c["Wc"], c["lens"], c["h0"], c["dh_T"], c["d_outs"] if outs else None)
        assert float((dxp - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_own_witnesses_change_nothing():
    """a witness equal to the reference's own float32 tape: logs at float32 rounding, outputs within 1e-6 (a rounding
    flip of the float32 copy aside, none on this case)"""
    case = (64, 33, 3)
    c, ref, _, dxp = _rounded(case)
    wit = {"hs": ref["hs"].float(), "rh": ref["rh"].float(), "dxp": dxp[False].float()}
    got, cell = Q.forward(c, wit=wit)
    assert float((got["hs"] - ref["hs"]).abs().max()) <= 1e-6
    d, cell = Q.backward(c, wit=wit)
    assert float((d - dxp[False]).abs().max()) <= 1e-6 * float(dxp[False].abs().max())
    assert 0.0 < cell.witness_distance() <= 1e-6


@pytest.mark.parametrize("case", Q.CASES)
def test_rounding_is_visible_at_ten_times_the_gpu_bound(case):
    c = _rounded(case)[0]
    plain = Q.forward(c, rounding=False)[0]
    dxp = {o: Q.backward(c, o, rounding=False)[0] for o in (False, True)}
    fwd, bwd = _distances(case, plain, dxp)
    print("GRU-BF16-REF %-16s unrounded: hs %.1f x bound, dxp %.1f x bound" % (case, fwd, bwd))
    assert fwd >= MARGIN and bwd >= MARGIN, (fwd, bwd)


@pytest.mark.parametrize("case", Q.CASES)
def test_truncation_is_visible_at_ten_times_the_gpu_bound(case):
    c = _rounded(case)[0]
    with Q.conversion(R.truncate_bf16):
        trunc = Q.forward(c)[0]
        dxp = {o: Q.backward(c, o)[0] for o in (False, True)}
    fwd, bwd = _distances(case, trunc, dxp)
    print("GRU-BF16-REF %-16s truncated: hs %.1f x bound, dxp %.1f x bound" % (case, fwd, bwd))
    assert fwd >= MARGIN and bwd >= MARGIN, (fwd, bwd)
