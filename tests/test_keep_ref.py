"""CPU checks of the keep-bit stream's restatement (tests/keep_ref.py) and of the seeded entry points' refusals, which
happen before any HIP call."""
import numpy as np
import pytest

from tests import keep_ref as K

SEEDS = (123, 9, 77)
OFFSETS = (0, (3 << 40) + 49380, (1 << 40) + 3)


@pytest.fixture(scope="module")
def built(repo_root):
    import __graft_entry__ as g
    g.build()
    from vqa_transfer_externaldata_amd import _lib
    return _lib


@pytest.mark.parametrize("offset", OFFSETS)
def test_a_split_range_equals_the_whole_range(offset):
    whole = K.keep_bits(1000, 123, offset, 0.8)
    for cut in (1, 4, 333, 998):
        parts = np.concatenate([K.keep_bits(cut, 123, offset, 0.8), K.keep_bits(1000 - cut, 123, offset + cut, 0.8)])
        assert np.array_equal(parts, whole), cut


def test_offsets_that_are_no_multiple_of_four():
    whole = K.keep_bits(1 << 12, 9, 0, 0.5)
    for off in (1, 2, 3, 5, 4095 - 64):
        assert np.array_equal(K.keep_bits(64, 9, off, 0.5), whole[off:off + 64]), off
    # the four positions of a group share one hash: four distinct 16-bit fields of it
    assert len({tuple(K.keep_bits(4, 77, 4 * g, 0.5)) for g in range(64)}) > 4


def test_keep_one_keeps_everything_and_keep_zero_nothing():
    assert K.keep_bits(1 << 16, 9, 0, 1.0).min() == 1
    assert K.keep_bits(1 << 16, 9, 3, 0.0).max() == 0
    assert (K.keep_thr(1.0), K.keep_thr(0.5), K.keep_thr(0.8), K.keep_thr(-1.0)) == (65536, 32768, 52428, 0)


@pytest.mark.parametrize("keep", [0.8, 0.5])
def test_kept_fraction_is_binomial_around_the_threshold(keep):
    """65536 draws: within 4 binomial standard deviations of floor(keep 65536) / 65536 (the largest of the 18 cases is 1.7)"""
    n = 65536
    p = K.keep_thr(keep) / 65536.0
    sd = np.sqrt(p * (1 - p) / n)
    for seed in SEEDS:
        for off in OFFSETS:
            frac = K.keep_bits(n, seed, off, keep).mean()
            assert abs(frac - p) <= 4 * sd, (seed, off, (frac - p) / sd)


P = 16      # a non-NULL, 16-byte aligned stand-in for a device pointer: nothing is dereferenced before the checks


def _calls(lib, offset, null):
    """the five seeded entry points, each with `offset` and (null) its first required pointer missing"""
    a = None if null else P
    return {
        "vqa_attn_pool_fwd_seeded": lib.vqa_attn_pool_fwd_seeded(a, P, P, 0, P, P, P, 123, offset, 0.8, P, P, 2, 1, 5, 8, 12, None),
        "vqa_attn_pool_bwd_seeded": lib.vqa_attn_pool_bwd_seeded(a, P, P, P, 0, P, P, 123, offset, 0.8, P, P, P, P, 2, 1, 5, 8, 12,
                                                                 None),
        "vqa_ln_act_fwd_seeded": lib.vqa_ln_act_fwd_seeded(a, P, P, 123, offset, 0.5, P, P, P, 2, 1, 8, 0, None),
        "vqa_ln_act_bwd_seeded": lib.vqa_ln_act_bwd_seeded(a, P, P, P, P, P, 123, offset, 0.5, P, P, P, P, 2, 1, 8, 0, None),
        "vqa_ln_relu_att_bwd_seeded": lib.vqa_ln_relu_att_bwd_seeded(a, P, P, 123, offset, 0.8, *([P] * 11), 2, 1, 36, 1024, 2048,
                                                                     None),
    }


def test_seeded_entry_points_refuse_before_any_hip_call(built):
    lib = built.load()
    ARG, ALIGN, UNSUPPORTED = -1, -2, -4
    assert _calls(lib, 2, False) == {k: ALIGN for k in _calls(lib, 2, False)}
    assert _calls(lib, 0, True) == {k: ARG for k in _calls(lib, 0, True)}
    assert len(_calls(lib, 0, True)) == 5
    # a row length that is no multiple of 4, keep_prob <= 0, several queries per memory
    assert lib.vqa_ln_act_fwd_seeded(P, P, P, 123, 0, 0.5, P, P, P, 2, 1, 6, 0, None) == ALIGN
    assert lib.vqa_attn_pool_fwd_seeded(P, P, P, 0, P, P, P, 123, 0, 0.8, P, P, 2, 1, 5, 6, 12, None) == ALIGN
    assert lib.vqa_ln_act_bwd_seeded(P, P, P, P, P, P, 123, 0, 0.0, P, P, P, P, 2, 1, 8, 0, None) == ARG
    assert lib.vqa_attn_pool_fwd_seeded(P, P, P, 0, P, P, P, 123, 0, 0.8, P, P, 2, 5, 5, 8, 12, None) == UNSUPPORTED
    assert lib.vqa_attn_pool_bwd_seeded(P, P, P, P, 0, P, P, 123, 0, 0.8, P, P, P, P, 2, 5, 5, 8, 12, None) == UNSUPPORTED
    assert lib.vqa_ln_relu_att_bwd_seeded(P, P, P, 123, 0, 0.8, *([P] * 11), 2, 5, 36, 1024, 2048, None) == UNSUPPORTED


def test_a_seeded_site_with_a_mask_pointer_is_refused(built):
    import ctypes as C
    lib = built.load()
    d = built.Dims(B=4, R=6, D=24, H=16, T=7, W=12, A=21, Vq=30, N_img=9, model_type=0, keep_att=0.8, keep_joint=0.5,
                   inv_global_batch=0.25)
    ws = (C.c_char * 64)()
    for name, bit in built.KEEP_SITE.items():
        b = built.Batch(keep_seeded=bit, **{name: P})
        assert lib.vqa_fusion_forward(C.byref(d), C.byref(built.Params()), C.byref(b), ws, 64, 0, None) == -1, name
    assert lib.vqa_fusion_forward(C.byref(d), C.byref(built.Params()), C.byref(built.Batch(keep_seeded=32)), ws, 64, 0, None) == -1
    # (no mask pointer: the call gets as far as the workspace check)
    assert lib.vqa_fusion_forward(C.byref(d), C.byref(built.Params()), C.byref(built.Batch(keep_seeded=31)), ws, 64, 0, None) == -5
