"""Float64 reference of the extractor's bf16 mode (vfeat.ResNetV1(precision="bf16")).

TEST INFRASTRUCTURE ONLY.  Built on oracle/conv_oracle.py (the float64 convolution, pooling and network) and on
tests/bf16_ref.py (round_bf16 / truncate_bf16 of float32 operands).  Two layers:

  * the op: conv_ref = relu(conv(x^, w^) * scale + shift + res) in float64 on operands that are ALREADY bf16 values, with
    conv_yardstick = |scale| (|x^| * |w^|) + |shift| + |res| as the per-element measure of what one f32 rounding may cost;
  * the trunk: conv_oracle.resnet_v1 with the roundings of the contract in the places of the contract (filters once,
    the max-pool output, every convolution's stored output except the last).  With rounding=False it IS
    conv_oracle.resnet_v1 (tests/test_conv_bf16_ref.py holds it to that).

Criterion of the op, tolerance T (op_check):
  f32 output:  |got - v| <= T s
  bf16 output: round(act(u - T s)) <= got <= round(act(u + T s)), u the value before the activation: true exactly when got
               is the nearest-even rounding of SOME value within T s of the reference.  No element is skipped.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import conv_oracle as CO
from tests import bf16_ref as BR

# Worst |got - v| / s over every f32-output case of tests/test_gpu_vfeat_bf16.py::test_conv_op on the MI355X
# (profiles/r13_vfeat_bf16_bench.txt): OP_TOL_MEASURED; OP_TOL = 3 x that, the margin bf16_ref.OP_TOL gives another legal
# f32 summation order.
OP_TOL_MEASURED = 1.131e-7      # measured: the 1x1, Ci 2048 -> Co 512 case (64 k tiles), f32 output
OP_TOL = 3 * OP_TOL_MEASURED


def round_bf16_f64(a):
    """float64 array rounded DIRECTLY to the nearest bf16 (ties to even), returned as float64.  (Going through float32
    first rounds twice; a bracket bound must not.)  Finite values of bf16's normal range or zero, which is all the tests
    produce."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    bits = a.view(np.uint64)
    drop = np.uint64(45)                                   # 52 mantissa bits of float64 -> 7 of bf16
    lsb = (bits >> drop) & np.uint64(1)
    out = (bits + np.uint64((1 << 44) - 1) + lsb) & ~np.uint64((1 << 45) - 1)
    return out.view(np.float64).reshape(a.shape)


def round_operand(a):
    """a float32-representable array rounded to bf16 by bf16_ref.round_bf16 (the conversion torch and the host packer
    use), as float64"""
    return BR.round_bf16(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).double().numpy()


def to_bf16_bits(a):
    """bf16-valued float array -> torch.bfloat16 tensor (exact)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def pad_same(k):
    """slim conv2d_same / 'SAME' at stride 1 for an odd k: (k - 1) split begin / end"""
    beg = (k - 1) // 2
    return ((beg, k - 1 - beg), (beg, k - 1 - beg))


def _pre(xh, wh, stride, pad, scale, shift, res):
    u = CO.conv2d_nhwc(np.asarray(xh, np.float64), np.asarray(wh, np.float64), stride, pad)
    if scale is not None:
        u = u * np.asarray(scale, np.float64)
    if shift is not None:
        u = u + np.asarray(shift, np.float64)
    if res is not None:
        u = u + np.asarray(res, np.float64)
    return u


def conv_ref(xh, wh, stride, pad, scale, shift, res, relu):
    """v = [relu](conv(x^, w^) * scale + shift + res) in float64.  xh [B,H,W,Ci] and res [B,Ho,Wo,Co] hold bf16 values,
    wh HWIO holds bf16 values, pad = ((top, bottom), (left, right))."""
    u = _pre(xh, wh, stride, pad, scale, shift, res)
    return np.maximum(u, 0) if relu else u


def conv_yardstick(xh, wh, stride, pad, scale, shift, res):
    """s = |scale| (|x^| * |w^|) + |shift| + |res|"""
    return _pre(np.abs(xh), np.abs(wh), stride, pad, None if scale is None else np.abs(scale),
                None if shift is None else np.abs(shift), None if res is None else np.abs(res))


def bracket(u, s, tol, relu):
    """(lo, hi) of the bf16-output criterion from the value before the activation"""
    act = (lambda t: np.maximum(t, 0)) if relu else (lambda t: t)
    return round_bf16_f64(act(u - tol * s)), round_bf16_f64(act(u + tol * s))


def op_check(got, u, s, tol, relu, out_f32):
    """(number of elements outside the criterion, worst |got - v| / s).  got: the kernel's output as a float64 array, u
    the reference BEFORE the activation, s the yardstick."""
    got = np.asarray(got, np.float64)
    v = np.maximum(u, 0) if relu else u
    ratio = float((np.abs(got - v) / np.maximum(s, 1e-300)).max())
    if out_f32:
        bad = np.abs(got - v) > tol * s
    else:
        lo, hi = bracket(u, s, tol, relu)
        bad = (got < lo) | (got > hi)
    return int(bad.sum()), ratio


def op_case(k, Ci, Co, B, H, W, seed, residual_hw=None):
    """seeded normal operands of an op test, already rounded to bf16: x [B,H,W,Ci], HWIO filter (He scale), folded
    BatchNorm scale / shift (f32), and -- when residual_hw = (Ho, Wo) is given -- a residual [B,Ho,Wo,Co]"""
    g = torch.Generator().manual_seed(seed)
    x = BR.round_bf16(torch.randn(B, H, W, Ci, generator=g)).numpy()
    w = BR.round_bf16(torch.randn(k, k, Ci, Co, generator=g) * float(np.sqrt(2.0 / (k * k * Ci)))).numpy()
    scale = (1 + 0.1 * torch.randn(Co, generator=g)).numpy()
    shift = (0.1 * torch.randn(Co, generator=g)).numpy()
    res = None
    if residual_hw is not None:
        res = BR.round_bf16(torch.randn(B, residual_hw[0], residual_hw[1], Co, generator=g)).numpy()
    return x, w, scale, shift, res


def im2col(x, kh, kw, stride, pad):
    """[B*Ho*Wo, kh*kw*Ci] with k = (ky, kx, ci): the rows conv_oracle.conv2d_nhwc multiplies with the HWIO filter"""
    B, H, W, Ci = x.shape
    xp = np.pad(x, ((0, 0), pad[0], pad[1], (0, 0)))
    Ho, Wo = (xp.shape[1] - kh) // stride + 1, (xp.shape[2] - kw) // stride + 1
    cols = np.empty((B, Ho, Wo, kh, kw, Ci), x.dtype)
    for ky in range(kh):
        for kx in range(kw):
            cols[:, :, :, ky, kx, :] = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :]
    return cols.reshape(B * Ho * Wo, kh * kw * Ci), (B, Ho, Wo)


def conv_bf16_accumulate(xh, wh, stride, pad, ktile=32):
    """the WRONG accumulation (discrimination test): the running sum rounded to bf16 after every `ktile`-deep k tile"""
    kh, kw, Ci, Co = wh.shape
    cols, (B, Ho, Wo) = im2col(np.asarray(xh, np.float64), kh, kw, stride, pad)
    w2 = np.asarray(wh, np.float64).reshape(kh * kw * Ci, Co)
    acc = np.zeros((cols.shape[0], Co))
    for k0 in range(0, cols.shape[1], ktile):
        acc = round_bf16_f64(acc + cols[:, k0:k0 + ktile] @ w2[k0:k0 + ktile])
    return acc.reshape(B, Ho, Wo, Co)


def unpack_weight(packed, kh, kw, ci, co):
    """[Co][kh*kw*Ci] (the kernel's layout) -> HWIO"""
    return np.asarray(packed).reshape(co, kh, kw, ci).transpose(1, 2, 3, 0)


# ----------------------------------------------------------------------------- trunk
def trunk_ref(images, params, blocks, rounding=True, scope="resnet_v1_50"):
    """conv_oracle.resnet_v1 in float64 with the contract's roundings: the stem (mean subtraction, conv1, BatchNorm, ReLU)
    unrounded; the max-pool output rounded; every later filter rounded once; every later convolution's output (after
    BatchNorm, residual and ReLU) rounded, except the last one's."""
    r = round_bf16_f64 if rounding else (lambda t: t)
    p = {k: np.asarray(v, np.float64) for k, v in params.items()}
    images = np.asarray(images, np.float64)

    def bn(y, name):
        return CO.bn_inference(y, {k: p[name + "/BatchNorm/" + k] for k in ("gamma", "beta", "moving_mean", "moving_variance")},
                               CO.SLIM_BN_EPS)

    x = images - np.asarray(CO.ENC_I_MEAN, np.float64)
    x = np.maximum(bn(CO.conv2d_same(x, p[scope + "/conv1/weights"], 2), scope + "/conv1"), 0)
    x = r(CO.max_pool_3x3_s2_same(x))
    units = [(name, i, u) for name, base, n, stride in blocks for i, u in enumerate(CO.block_units(base, n, stride))]
    for j, (name, i, (depth, db, s)) in enumerate(units):
        pre = "%s/%s/unit_%d/bottleneck_v1" % (scope, name, i + 1)
        last = j == len(units) - 1

        def cbn(inp, cname, stride, same=False):
            w = r(p[pre + "/" + cname + "/weights"])
            y = CO.conv2d_same(inp, w, stride) if same else CO.conv2d_nhwc(CO.subsample(inp, stride), w, 1)
            return bn(y, pre + "/" + cname)

        shortcut = CO.subsample(x, s) if depth == x.shape[-1] else r(cbn(x, "shortcut", s))
        h = r(np.maximum(cbn(x, "conv1", 1), 0))
        h = r(np.maximum(cbn(h, "conv2", s, same=True), 0))
        y = np.maximum(shortcut + cbn(h, "conv3", 1), 0)
        x = y if last else r(y)
    return x


def max_distance(got, want):
    """max |got - want| / max |want|"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


def trunk_case(blocks_name, width_div, units, size, seed=6):
    """the network cases of tests/test_gpu_vfeat.py::test_resnet_stack_matches_oracle: (params f32, blocks, images f32)"""
    rng = np.random.default_rng(seed)
    base = CO.BLOCKS_R50_B3 if blocks_name == "R50_B3" else CO.BLOCKS_R50_FULL
    full = [(n, b, units, s) for (n, b, u, s) in base]
    p = CO.init_resnet_params(rng, full, dtype=np.float32, width_div=width_div)
    blocks = [(n, b // width_div, u, s) for (n, b, u, s) in full]
    img = rng.uniform(0, 255, size=(2, size, size + 16, 3)).astype(np.float32)
    return p, blocks, img


TRUNK_CASES = [("R50_B3", 2, 2, 96), ("R50_FULL", 2, 1, 80)]


# ----------------------------------------------------------------------------- model heads
def model_heads(enc, normal_box, p, v_dim=512, roi_sz=5):
    """what conv_oracle.model_vfeat_resnet and conv_oracle.model_vfeat do AFTER the trunk, on a given trunk output:
    (V_ft of vfeat_resnet [B,n,C], V_ft of vfeat [B,n,v_dim]) in float64"""
    enc = np.asarray(enc, np.float64)
    box = np.asarray(normal_box, np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    B, n = box.shape[:2]
    v_resnet = CO.roi_pool(enc, box, 1, 1).reshape(B, n, enc.shape[-1])

    def conv_bn_relu(x, scope, pad_same_):
        w = p[scope + "/conv2d/weights"]
        k = w.shape[0]
        pad = (CO.same_pad(x.shape[1], k, 1), CO.same_pad(x.shape[2], k, 1)) if pad_same_ else ((0, 0), (0, 0))
        y = CO.bn_inference(CO.conv2d_nhwc(x, w, 1, pad), {kk: p[scope + "/BatchNorm/" + kk]
                                                           for kk in ("gamma", "beta", "moving_mean", "moving_variance")},
                            CO.LAYERS_BN_EPS)
        return np.maximum(y, 0)

    low = conv_bn_relu(enc, "I_reduce_dim/conv2d", True)
    flat = CO.roi_pool(low, box, roi_sz, roi_sz).reshape(B * n, roi_sz, roi_sz, v_dim)
    v = conv_bn_relu(conv_bn_relu(flat, "I2V/conv2d_1", False), "I2V/conv2d_1", False)
    return v_resnet, v.reshape(B, n, v_dim)


def model_case(seed=7):
    """the small case of tests/test_gpu_vfeat.py::test_vfeat_models_match_oracle: (params f32, blocks, images, boxes, v_dim)"""
    rng = np.random.default_rng(seed)
    full = [(n, b, 1, s) for (n, b, u, s) in CO.BLOCKS_R50_B3]
    p = CO.init_resnet_params(rng, full, dtype=np.float32, width_div=2)
    blocks = [(n, b // 2, u, s) for (n, b, u, s) in full]
    p = CO.init_vfeat_head_params(rng, p, blocks[-1][1] * 4, 64)
    img = rng.uniform(0, 255, size=(2, 128, 128, 3)).astype(np.float32)
    box = CO.make_boxes(rng, 2, 7)
    return p, blocks, img, box, 64
