"""Float64 reference of the f32 region-feature extractor kernels of include/vqa_hot.h (vqa_conv2d_nhwc: csrc/gemm_f32.hip
and csrc/gemm_shortk.hip; vqa_conv2d_nhwc_bwd: csrc/conv_bwd.hip; vqa_crop_and_resize_nhwc, vqa_maxpool3x3s2_same_nhwc,
vqa_subsample_nhwc, vqa_pad_c3c4_nhwc: csrc/conv_ops.hip), the data, the guarded buffers and the comparators of their
op-level tests, and the case matrix that crosses every route of the two dispatchers with every edge of their loops.

conv_fwd evaluates  y = [relu]( conv(x, w) * scale[co] + shift[co] + residual )  in float64 as a direct sum over the
filter taps (for every tap the output pixels whose tap lies inside the image take x[pixel + tap] @ w[tap]; no column
matrix is built, so it is not a restatement of the kernels) and returns beside it the magnitude sum
scale_y = conv(|x|, |w|) |scale| + |shift| + |residual| that a rounding error is proportional to.  conv_bwd evaluates
the header's formulas for dx, dw, dshift and dresidual the same way, g taken from the y handed in (mask y > 0: 0.0 and
-0.0 are both off), each with its magnitude sum.  crop_and_resize evaluates the sampling coordinates in float32 in the
kernel's and TensorFlow's expression order and the bilinear blend in float64; max-pool, subsample and the 3 -> 4 channel
padding are bit-exact restatements.

Two kinds of data for every convolution case:
  exact   x, w, residual, dy are integers in [-3, 3], shift an integer in [-5, 5], scale in {-2, -1, -0.5, 0.5, 1, 2}, all
          stored as float32.  Every partial sum of every summation order is a multiple of 1/2 (dz = g * scale is one and
          w an integer) whose magnitude the reference bounds per case (exact_bounds) and asserts to be below 2^23, so
          twice any partial sum is an integer below 2^24: every order is exact and the comparator is equality with the
          float64 value whatever the tile, route, slab or chunk count.
  real    standard normal operands, judged element by element:  |got - ref64| <= min(RT[output], n U) * scale, U = 2^-24.
          n counts the roundings between the exact products and the stored float, for ANY summation order:
            y        n = K + 8        K = kh kw Ci fused multiply-adds (one rounding each), the multiply by scale, the
                                      additions of shift and residual (3), and up to 4 partial-sum combines a tile's k
                                      groups or slabs may add, +1 spare: the bound of tests/gemm_ref.py with S = 1
            dx       n = Co + kh kw + 6   the product g * scale (1), Co fused multiply-adds of dz W^T, at most kh kw
                                      additions of the col2im gather, up to 4 k-group combines of the GEMM
            dw       n = B Ho Wo + B + 16 + 2   g * scale (1), one fused multiply-add per output pixel, one accumulation
                                      per chunk of images (at most B chunks), the slab sums of an automatic split-K (the
                                      dispatcher's cap is 16), +1 spare
            dshift   n = B Ho Wo + 4  one addition per output pixel in four strided partial sums and their 3 combines
            dresidual                 no rounding: dy or 0, compared bit for bit
          RT is measured, not chosen: this reference evaluated in float32 on the CPU in the two extreme orders a kernel
          can take (sequential over the summed index; 8-wide chunks summed, then combined), worst |ref32 - ref64| / scale
          over every `real` case of the matrix, times 8 -- the margin the project's references give a change of summation
          order.  tests/test_conv_reference.py measures it, holds this table to the live measurement and holds both
          float32 evaluations inside the bound.  It is never measured from a kernel.

  output   float32 worst   RT = 8x    at
  y        2.617e-07       2.09e-06   e-M65-2x4-ci4-co132-s1-p01-b5-1x13-o1x13 (seq)
  dx       2.528e-07       2.02e-06   j-7x7-ci4-co16-s3-p00-b2-10x11-o1x1 (seq)
  dw       2.207e-07       1.77e-06   j-7x7-ci4-co16-s1-p11-b2-10x11-o6x7 (seq)
  dshift   1.244e-07       9.95e-07   j-1x3-ci8-co16-s3-p20-b2-9x8-o5x2 (seq)
RT is 35 U for y (so n U is the smaller term up to K = 27 and RT is above), 34 U for dx, 30 U for dw, 17 U for dshift.

Crop and resize.  `exact` cases: H - 1 and W - 1 in {0, 4, 8}, box corners in eighths and crop - 1 in {0, 1, 2, 4}, so
every coordinate and weight is dyadic, the feature map is integer and the comparator is equality.  `real` cases:
|got - ref64| <= CROP_C U (|tl| + |tr| + |bl| + |br|) with CROP_C = 7: the kernel blends with three lerps
a + (b - a) l, each of at most three roundings (subtract, multiply, add; a fused multiply-add has fewer), 0 <= l < 1.
A lerp of exact inputs errs by at most 2 U |b - a| l + U |result| <= 3 U (|a| + |b|) to first order; the two horizontal
lerps feed the vertical one with weights 1 - ly and ly, which passes on at most 3 U (|tl| + |tr| + |bl| + |br|), and
the vertical lerp adds 3 U (|t| + |bt|) of its own: 6 U of the corner sum, and the second-order terms stay far below one
more U.  The weights lx, ly are exact (in_y - floor(in_y) is exact in float32) and the coordinates are the float32
values of the kernel's own expression, which the reference evaluates in the same order.  No case has a box_ind outside
[0, B) or a non-finite box: those read out of bounds.

Buffers: every input sits between two NaN guards of GUARD floats (so a loader that reads before or past an operand
shows as NaN in the result), every output is NaN-filled between two NaN guards; after the call the guards are still
NaN, after an accepted call no output element is NaN, after a refused call the whole output is still NaN.

The case matrix lives here, one builder per group (cases_a .. cases_l); matrix() returns all of it.  Shapes are small
(B <= 5, H, W <= 13) with one exception: M = B Ho Wo = 129 = 3 * 43 has no factorisation inside those limits, so that
one tile-edge shape is 3 images of 1 x 43.  M = 1 needs B = 1; every other tile-edge shape has B > 1.

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import itertools
import typing
import zlib

import numpy as np

U = 2.0 ** -24
OK, ERR_ARG, ERR_ALIGN, ERR_LAUNCH, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3, -4, -5
GUARD = 64                      # floats of NaN on either side of every buffer (a multiple of 16 bytes)
CROP_C = 7
F32_MIN = np.float32(np.finfo(np.float32).tiny)
F32_DENORM_MIN = np.float32(1.401298464324817e-45)

# 8x the measured float32 error of this reference (tests/test_conv_reference.py holds both to the live measurement)
MEASURED = {
    "y": (2.617e-07, "e-M65-2x4-ci4-co132-s1-p01-b5-1x13-o1x13 (seq)"),
    "dx": (2.528e-07, "j-7x7-ci4-co16-s3-p00-b2-10x11-o1x1 (seq)"),
    "dw": (2.207e-07, "j-7x7-ci4-co16-s1-p11-b2-10x11-o6x7 (seq)"),
    "dshift": (1.244e-07, "j-1x3-ci8-co16-s3-p20-b2-9x8-o5x2 (seq)"),
}
RT = {k: 8 * v[0] for k, v in MEASURED.items()}
SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


# -------------------------------------------------------------------------------------------------------------- cases
def full_extent(size, k, stride, pad):
    """output extent of a convolution padded by `pad` on both sides"""
    return (size + 2 * pad - k) // stride + 1


class Conv(typing.NamedTuple):
    """a call of vqa_conv2d_nhwc"""
    group: str
    name: str
    B: int
    Hi: int
    Wi: int
    Ci: int
    kh: int
    kw: int
    Co: int
    stride: int = 1
    pad: tuple = (0, 0)          # (pad_t, pad_l)
    out: typing.Optional[tuple] = None   # (Ho, Wo); None: the full extent under the same padding at the bottom / right
    scale: bool = True
    shift: bool = True
    residual: bool = True
    relu: int = 1
    ccfg: int = -1               # vqa_conv_set_config
    gcfg: int = -1               # vqa_gemm_set_config
    shortk: int = -1             # vqa_gemm_shortk_set_mode
    expect: int = OK
    x_off: int = 0               # floats past a 16-byte boundary
    null: str = ""               # refusals: the pointer passed as NULL ("x", "w", "y")
    zero_last_column: bool = False   # conv1's [7, 8, 4] filter: the eighth tap of every row is zero
    route: str = ""              # the route the dispatcher takes (what the worst-error table is keyed by)
    kinds: tuple = ("exact", "real")
    salt: int = 0

    def id(self):
        return self.name

    @property
    def Ho(self):
        return self.out[0] if self.out else full_extent(self.Hi, self.kh, self.stride, self.pad[0])

    @property
    def Wo(self):
        return self.out[1] if self.out else full_extent(self.Wi, self.kw, self.stride, self.pad[1])

    @property
    def M(self):
        return self.B * self.Ho * self.Wo

    @property
    def K(self):
        return self.kh * self.kw * self.Ci

    @property
    def plain(self):
        """the dispatcher's test for the 1x1 / stride-1 route"""
        return (self.kh == 1 and self.kw == 1 and self.stride == 1 and self.pad == (0, 0) and
                self.Ho == self.Hi and self.Wo == self.Wi)


class Bwd(typing.NamedTuple):
    """a call of vqa_conv2d_nhwc_bwd"""
    group: str
    name: str
    B: int
    Hi: int
    Wi: int
    Ci: int
    kh: int
    kw: int
    Co: int
    stride: int = 1
    pad: tuple = (0, 0)
    out: typing.Optional[tuple] = None
    scale: bool = True
    relu: int = 1
    y_null: bool = False         # relu == 0 only
    outs: tuple = ("dx", "dw", "dshift", "dresidual")    # the others are passed as NULL
    chunk: int = 0               # the workspace is vqa_conv2d_bwd_workspace_floats(..., chunk); 0: B
    ws_short: int = 0            # floats taken off that workspace
    plant: bool = False          # y carries planted 0.0, -0.0, the smallest denormal and the smallest normal float
    expect: int = OK
    route: str = ""
    kinds: tuple = ("exact", "real")
    salt: int = 0

    def id(self):
        return self.name

    Ho = Conv.Ho
    Wo = Conv.Wo
    M = Conv.M
    K = Conv.K

    @property
    def pointwise(self):
        return (self.kh == 1 and self.kw == 1 and self.stride == 1 and self.pad == (0, 0) and
                self.Ho == self.Hi and self.Wo == self.Wi)

    @property
    def chunks(self):
        """images per chunk the dispatcher's search B, B/2, B/4, ... arrives at"""
        want, c = self.chunk or self.B, self.B
        while c > want:
            c //= 2
        return c


class Crop(typing.NamedTuple):
    name: str
    B: int
    H: int
    W: int
    C: int
    ch: int
    cw: int
    boxes: str = "all"           # "all": every box of BOXES (+ the non-dyadic ones for `real`); "none": n_boxes = 0
    kinds: tuple = ("exact", "real")

    def id(self):
        return self.name


class Pool(typing.NamedTuple):
    name: str
    op: str                      # "maxpool", "subsample", "pad"
    B: int
    Hi: int
    Wi: int
    C: int
    factor: int = 1
    negative: bool = False       # an all-negative input (the padding must never win the maximum)
    expect: int = OK

    def id(self):
        return self.name


# --------------------------------------------------------------------------------------------------------------- data
_DATA: dict = {}
_REF: dict = {}


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _draw(rng, kind, *shape):
    if kind == "exact":
        return rng.randint(-3, 4, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _shape_key(c):
    return (c.B, c.Hi, c.Wi, c.Ci, c.kh, c.kw, c.Co, c.stride, c.pad, c.Ho, c.Wo, c.salt)


def operands(c, kind):
    """{x [B,Hi,Wi,Ci], w [kh,kw,Ci,Co], scale [Co], shift [Co], residual [B,Ho,Wo,Co], dy [B,Ho,Wo,Co]} (float32) of a
    Conv or a Bwd; cases of one shape share them"""
    key = (kind, bool(getattr(c, "zero_last_column", False))) + _shape_key(c)
    if key not in _DATA:
        rng = _rng(*key)
        d = {"x": _draw(rng, kind, c.B, c.Hi, c.Wi, c.Ci), "w": _draw(rng, kind, c.kh, c.kw, c.Ci, c.Co)}
        if kind == "exact":
            d["scale"] = rng.choice(np.array(SCALES, np.float32), size=c.Co)
            d["shift"] = rng.randint(-5, 6, size=c.Co).astype(np.float32)
        else:
            d["scale"] = _draw(rng, kind, c.Co)
            d["shift"] = _draw(rng, kind, c.Co)
        d["residual"] = _draw(rng, kind, c.B, c.Ho, c.Wo, c.Co)
        d["dy"] = _draw(rng, kind, c.B, c.Ho, c.Wo, c.Co)
        if key[1]:
            d["w"][:, -1] = 0
        _DATA[key] = d
    return _DATA[key]


# ---------------------------------------------------------------------------------------------------------- reference
def _taps(Hi, Wi, kh, kw, stride, pad_t, pad_l, Ho, Wo):
    """for every filter tap that lies inside the image for some output pixel: (ky, kx, oy, iy, ox, ix), the output rows
    and columns it is inside for and the input rows and columns it reads there"""
    oy, ox = np.arange(Ho), np.arange(Wo)
    for ky in range(kh):
        iy = oy * stride - pad_t + ky
        my = (iy >= 0) & (iy < Hi)
        for kx in range(kw):
            ix = ox * stride - pad_l + kx
            mx = (ix >= 0) & (ix < Wi)
            if my.any() and mx.any():
                yield ky, kx, oy[my][:, None], iy[my][:, None], ox[mx][None, :], ix[mx][None, :]


def conv_sum(x, w, stride, pad_t, pad_l, Ho, Wo):
    """conv(x, w) [B,Ho,Wo,Co] in float64: zero padding, taps outside the image contribute nothing"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, Hi, Wi, _ = x.shape
    kh, kw, _, Co = w.shape
    out = np.zeros((B, Ho, Wo, Co))
    for ky, kx, oy, iy, ox, ix in _taps(Hi, Wi, kh, kw, stride, pad_t, pad_l, Ho, Wo):
        out[:, oy, ox, :] += x[:, iy, ix, :] @ w[ky, kx]
    return out


def conv_fwd(x, w, stride, pad_t, pad_l, Ho, Wo, scale=None, shift=None, residual=None, relu=0):
    """(y, scale_y) of vqa_conv2d_nhwc in float64"""
    z = conv_sum(x, w, stride, pad_t, pad_l, Ho, Wo)
    s = conv_sum(np.abs(x), np.abs(w), stride, pad_t, pad_l, Ho, Wo)
    if scale is not None:
        z, s = z * np.asarray(scale, np.float64), s * np.abs(np.asarray(scale, np.float64))
    if shift is not None:
        z, s = z + np.asarray(shift, np.float64), s + np.abs(np.asarray(shift, np.float64))
    if residual is not None:
        z, s = z + np.asarray(residual, np.float64), s + np.abs(np.asarray(residual, np.float64))
    if relu:
        z = np.maximum(z, 0.0)
    return z, s


def relu_mask(y):
    """the header's mask: y > 0 (0.0, -0.0 and anything negative are off; the smallest positive float is on)"""
    return np.asarray(y) > 0


def conv_bwd(x, w, stride, pad_t, pad_l, Ho, Wo, scale, y, relu, dy):
    """{dx, dw, dshift, dresidual: (value, magnitude sum)} of vqa_conv2d_nhwc_bwd in float64"""
    x, w, dy = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(dy, np.float64)
    B, Hi, Wi, Ci = x.shape
    kh, kw, _, Co = w.shape
    g = dy * relu_mask(y) if relu else dy
    dz = g * np.asarray(scale, np.float64) if scale is not None else g
    ax, aw, adz = np.abs(x), np.abs(w), np.abs(dz)
    dx, sdx = np.zeros_like(x), np.zeros_like(x)
    dw, sdw = np.zeros_like(w), np.zeros_like(w)
    for ky, kx, oy, iy, ox, ix in _taps(Hi, Wi, kh, kw, stride, pad_t, pad_l, Ho, Wo):
        dx[:, iy, ix, :] += dz[:, oy, ox, :] @ w[ky, kx].T
        sdx[:, iy, ix, :] += adz[:, oy, ox, :] @ aw[ky, kx].T
        dw[ky, kx] = np.einsum("bhwc,bhwo->co", x[:, iy, ix, :], dz[:, oy, ox, :])
        sdw[ky, kx] = np.einsum("bhwc,bhwo->co", ax[:, iy, ix, :], adz[:, oy, ox, :])
    return {"dx": (dx, sdx), "dw": (dw, sdw), "dshift": (g.sum((0, 1, 2)), np.abs(g).sum((0, 1, 2))),
            "dresidual": (g, np.abs(g))}


def _assert_exact(bound, what):
    """every partial sum is a multiple of 1/2 of magnitude <= bound: exact in float32 when 2 * bound < 2^24"""
    assert 2 * bound < 2 ** 24, "%s: partial sums up to %g are not exact in float32" % (what, bound)


def exact_bounds(c):
    """the largest magnitude a partial sum of any order can reach on `exact` data: {output: bound}"""
    taps = c.kh * c.kw
    return {"y": 2 * 9 * c.K + 5 + 3,                       # |scale| <= 2, |x w| <= 9, |shift| <= 5, |residual| <= 3
            "dx": 2 * 3 * 3 * c.Co * taps,                  # |dz| <= 6, |w| <= 3
            "dw": 3 * 6 * c.M, "dshift": 3 * c.M}


def fwd_flags(c, d):
    return (d["scale"] if c.scale else None, d["shift"] if c.shift else None, d["residual"] if c.residual else None)


def ref_fwd(c, kind):
    """(y64, scale_y) of a Conv"""
    key = ("fwd", kind, c.zero_last_column, c.scale, c.shift, c.residual, c.relu) + _shape_key(c)
    if key not in _REF:
        d = operands(c, kind)
        if kind == "exact":
            _assert_exact(exact_bounds(c)["y"], c.id())
        _REF[key] = conv_fwd(d["x"], d["w"], c.stride, c.pad[0], c.pad[1], c.Ho, c.Wo, *fwd_flags(c, d), relu=c.relu)
    return _REF[key]


def y_for_bwd(c, kind):
    """the y a Bwd case hands in: the forward reference (scale as the case has it, shift and residual present) rounded to
    float32, with 0.0, -0.0, the smallest denormal and the smallest normal float planted where the case asks"""
    d = operands(c, kind)
    y, _ = conv_fwd(d["x"], d["w"], c.stride, c.pad[0], c.pad[1], c.Ho, c.Wo, d["scale"] if c.scale else None,
                    d["shift"], d["residual"], relu=1)
    y = y.astype(np.float32)
    if c.plant:
        flat = y.reshape(-1)
        vals = (np.float32(0.0), np.float32(-0.0), F32_DENORM_MIN, F32_MIN)
        for i in range(min(flat.size, 16)):
            flat[(i * 7) % flat.size] = vals[i % 4]
    return y


def ref_bwd(c, kind):
    """{output: (value64, magnitude)} of a Bwd"""
    key = ("bwd", kind, c.scale, c.relu, c.plant) + _shape_key(c)
    if key not in _REF:
        d = operands(c, kind)
        if kind == "exact":
            for k, b in exact_bounds(c).items():
                if k != "y":
                    _assert_exact(b, "%s %s" % (c.id(), k))
        _REF[key] = conv_bwd(d["x"], d["w"], c.stride, c.pad[0], c.pad[1], c.Ho, c.Wo, d["scale"] if c.scale else None,
                             y_for_bwd(c, kind), c.relu, d["dy"])
    return _REF[key]


# ------------------------------------------------------------------------------------------- float32 evaluations (RT)
def im2col(x, kh, kw, stride, pad_t, pad_l, Ho, Wo):
    """[B*Ho*Wo, kh*kw*Ci] in x's dtype, zero outside the image (only the float32 evaluations use it)"""
    B, Hi, Wi, Ci = x.shape
    cols = np.zeros((B, Ho, Wo, kh * kw, Ci), x.dtype)
    for ky, kx, oy, iy, ox, ix in _taps(Hi, Wi, kh, kw, stride, pad_t, pad_l, Ho, Wo):
        cols[:, oy, ox, ky * kw + kx, :] = x[:, iy, ix, :]
    return cols.reshape(B * Ho * Wo, kh * kw * Ci)


def _mm32(A, B, order):
    """A @ B in float32, the inner index summed one by one ("seq") or in chunks of 8 that are then combined ("chunk8")"""
    A, B = A.astype(np.float32), B.astype(np.float32)
    n = A.shape[1]
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    if order == "seq":
        for k in range(n):
            acc += A[:, k, None] * B[k, None, :]
        return acc
    for k0 in range(0, n, 8):
        part = np.zeros_like(acc)
        for k in range(k0, min(n, k0 + 8)):
            part += A[:, k, None] * B[k, None, :]
        acc += part
    return acc


def fwd32(c, kind, order):
    d = operands(c, kind)
    scale, shift, residual = fwd_flags(c, d)
    acc = _mm32(im2col(d["x"], c.kh, c.kw, c.stride, c.pad[0], c.pad[1], c.Ho, c.Wo), d["w"].reshape(c.K, c.Co), order)
    if scale is not None:
        acc *= scale
    if shift is not None:
        acc += shift
    if residual is not None:
        acc += residual.reshape(c.M, c.Co)
    if c.relu:
        acc = np.maximum(acc, np.float32(0))
    return acc.reshape(c.B, c.Ho, c.Wo, c.Co)


def bwd32(c, kind, order):
    """{dx, dw, dshift} in float32"""
    d = operands(c, kind)
    g = d["dy"] * relu_mask(y_for_bwd(c, kind)).astype(np.float32) if c.relu else d["dy"]
    dz = (g * d["scale"] if c.scale else g).reshape(c.M, c.Co)
    W = d["w"].reshape(c.K, c.Co)
    dcols = _mm32(dz, W.T, order).reshape(c.B, c.Ho, c.Wo, c.kh * c.kw, c.Ci)
    dx = np.zeros((c.B, c.Hi, c.Wi, c.Ci), np.float32)
    for ky, kx, oy, iy, ox, ix in _taps(c.Hi, c.Wi, c.kh, c.kw, c.stride, c.pad[0], c.pad[1], c.Ho, c.Wo):
        dx[:, iy, ix, :] += dcols[:, oy, ox, ky * c.kw + kx, :]
    cols = im2col(d["x"], c.kh, c.kw, c.stride, c.pad[0], c.pad[1], c.Ho, c.Wo)
    dw = _mm32(cols.T, dz, order).reshape(c.kh, c.kw, c.Ci, c.Co)
    dshift = _mm32(np.ones((1, c.M), np.float32), g.reshape(c.M, c.Co), order)[0]
    return {"dx": dx, "dw": dw, "dshift": dshift}


def roundings(c, what):
    """n of the module docstring"""
    if what == "y":
        return c.K + 8
    if what == "dx":
        return c.Co + c.kh * c.kw + 6
    if what == "dw":
        return c.M + c.B + 16 + 2
    if what == "dshift":
        return c.M + 4
    raise KeyError(what)


def coefficient(c, what, rt=None):
    return min((RT if rt is None else rt)[what], roundings(c, what) * U)


def measure_rt(cases, check=False):
    """{output: (worst |ref32 - ref64| / scale over the `real` cases in both orders, where)}; check: every float32
    evaluation is also held to the comparator's bound"""
    worst = {k: (0.0, "") for k in MEASURED}
    seen = set()

    def note(what, c, order, r32, r64, scale):
        if check:
            compare(r32, r64, scale, "real", coefficient(c, what), "%s %s (%s)" % (c.id(), what, order))
        e = np.abs(r32.astype(np.float64) - r64)
        nz = scale > 0
        assert not e[~nz].any()
        x = float((e[nz] / scale[nz]).max()) if nz.any() else 0.0
        if x > worst[what][0]:
            worst[what] = (x, "%s (%s)" % (c.id(), order))

    for c in cases:
        if not isinstance(c, (Conv, Bwd)) or "real" not in c.kinds or c.expect != OK:
            continue
        if isinstance(c, Conv):
            key = ("fwd", c.zero_last_column, c.scale, c.shift, c.residual, c.relu) + _shape_key(c)
        else:
            key = ("bwd", c.scale, c.relu, c.plant) + _shape_key(c)
        if key in seen:
            continue
        seen.add(key)
        for order in ("seq", "chunk8"):
            if isinstance(c, Conv):
                r64, scale = ref_fwd(c, "real")
                note("y", c, order, fwd32(c, "real", order), r64, scale)
            else:
                r = ref_bwd(c, "real")
                for what, r32 in bwd32(c, "real", order).items():
                    note(what, c, order, r32, *r[what])
    return worst


# ------------------------------------------------------------------------------------------------- crop / pool / pad
BOXES = (                       # dyadic (eighths): [y1, x1, y2, x2]
    (0.0, 0.0, 1.0, 1.0),       # the whole image
    (0.25, 0.125, 0.75, 0.625),  # the interior
    (0.875, 0.75, 0.125, 0.25),  # reversed in both directions
    (-0.5, 0.25, 0.5, 1.5),     # half outside
    (1.5, 1.5, 2.5, 2.5),       # wholly outside: exact zeros
    (-2.0, -2.0, -1.0, -1.0),   # wholly outside on the other side
    (0.5, 0.5, 1.0, 1.0),       # the last sample lies exactly on H - 1 and W - 1
    (1.0, 1.0, 1.0, 1.0),       # every sample on the last pixel
)
BOXES_REAL = ((0.2, 0.3, 0.7, 0.9), (-0.3, 0.4, 0.6, 1.3), (0.9, 0.1, 0.15, 0.8))   # not dyadic: `real` only


def crop_operands(c, kind):
    """{fmap [B,H,W,C], boxes [n,4], box_ind int32 [n]}: every box on a shuffled, repeating, non-monotone box_ind"""
    key = ("crop", kind, c.B, c.H, c.W, c.C, c.boxes)
    if key not in _DATA:
        rng = _rng(*key)
        boxes = [] if c.boxes == "none" else list(BOXES) + (list(BOXES_REAL) if kind == "real" else [])
        boxes = np.array(boxes * 2, np.float32).reshape(-1, 4)
        ind = (np.arange(len(boxes)) * 3 + 1) % c.B if c.B > 1 else np.zeros(len(boxes))
        if len(boxes) > 3 and c.B > 1:
            ind[0], ind[1], ind[2], ind[3] = c.B - 1, 0, c.B - 1, c.B - 1     # descending, then repeated
        _DATA[key] = {"fmap": _draw(rng, kind, c.B, c.H, c.W, c.C), "boxes": boxes, "box_ind": ind.astype(np.int32)}
    return _DATA[key]


def crop_coords(boxes, H, W, ch, cw):
    """(in_y [n, ch], in_x [n, cw]) in float32, in the kernel's and TensorFlow's expression order"""
    f = np.float32
    n = len(boxes)
    in_y, in_x = np.zeros((n, ch), f), np.zeros((n, cw), f)
    for i in range(n):
        y1, x1, y2, x2 = (f(v) for v in boxes[i])
        hs = (y2 - y1) * f(H - 1) / f(ch - 1) if ch > 1 else f(0)
        ws = (x2 - x1) * f(W - 1) / f(cw - 1) if cw > 1 else f(0)
        for yy in range(ch):
            in_y[i, yy] = y1 * f(H - 1) + f(yy) * hs if ch > 1 else f(0.5) * (y1 + y2) * f(H - 1)
        for xx in range(cw):
            in_x[i, xx] = x1 * f(W - 1) + f(xx) * ws if cw > 1 else f(0.5) * (x1 + x2) * f(W - 1)
    assert in_y.dtype == f and in_x.dtype == f
    return in_y, in_x


def crop_and_resize(fmap, boxes, box_ind, ch, cw):
    """(out [n,ch,cw,C], the sum of the four corner magnitudes) of vqa_crop_and_resize_nhwc: extrapolation value 0"""
    fm = np.asarray(fmap, np.float64)
    B, H, W, C = fm.shape
    n = len(boxes)
    out, mag = np.zeros((n, ch, cw, C)), np.zeros((n, ch, cw, C))
    in_y, in_x = crop_coords(boxes, H, W, ch, cw)
    for i in range(n):
        b = int(box_ind[i])
        assert 0 <= b < B and np.isfinite(boxes[i]).all()
        for yy in range(ch):
            y = in_y[i, yy]
            if y < 0 or y > np.float32(H - 1):
                continue
            top, bot = int(np.floor(y)), int(np.ceil(y))
            ly = float(y) - top
            for xx in range(cw):
                x = in_x[i, xx]
                if x < 0 or x > np.float32(W - 1):
                    continue
                left, right = int(np.floor(x)), int(np.ceil(x))
                lx = float(x) - left
                tl, tr, bl, br = fm[b, top, left], fm[b, top, right], fm[b, bot, left], fm[b, bot, right]
                t = tl + (tr - tl) * lx
                bt = bl + (br - bl) * lx
                out[i, yy, xx] = t + (bt - t) * ly
                mag[i, yy, xx] = np.abs(tl) + np.abs(tr) + np.abs(bl) + np.abs(br)
    return out, mag


def maxpool3x3s2_same(x):
    """slim pool1: 3x3 / stride 2 / SAME, the extra padding element at the end, padding never wins; bit for bit"""
    B, Hi, Wi, C = x.shape
    Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
    pt, pl = max((Ho - 1) * 2 + 3 - Hi, 0) // 2, max((Wo - 1) * 2 + 3 - Wi, 0) // 2
    out = np.full((B, Ho, Wo, C), -np.inf, np.float32)
    for ky, kx, oy, iy, ox, ix in _taps(Hi, Wi, 3, 3, 2, pt, pl, Ho, Wo):
        out[:, oy, ox, :] = np.maximum(out[:, oy, ox, :], x[:, iy, ix, :])
    return out


def subsample(x, factor):
    return np.ascontiguousarray(x[:, ::factor, ::factor, :])


def pad_c3c4(x, mean):
    """(x - mean, 0): the subtraction in float32"""
    out = np.zeros(x.shape[:3] + (4,), np.float32)
    out[..., :3] = x - (np.zeros(3, np.float32) if mean is None else np.asarray(mean, np.float32))
    return out


def pool_input(c):
    rng = _rng("pool", c.op, c.B, c.Hi, c.Wi, c.C, c.negative)
    x = rng.standard_normal((c.B, c.Hi, c.Wi, 3 if c.op == "pad" else c.C)).astype(np.float32)
    return -np.abs(x) - np.float32(0.5) if c.negative else x


PAD_MEAN = (123.68, 116.78, 103.94)


def ref_pool(c, x):
    if c.op == "maxpool":
        return maxpool3x3s2_same(x)
    if c.op == "subsample":
        return subsample(x, c.factor)
    return pad_c3c4(x, PAD_MEAN)


# ------------------------------------------------------------------------------------------------------------ buffers
def guarded(arr, off=0):
    """the input `arr` flat between two NaN guards, `off` floats past a 16-byte boundary: (buffer, start)"""
    arr = np.ascontiguousarray(arr)
    flat = arr.reshape(-1)
    if arr.dtype == np.int32:    # box_ind: guards of a value no image has would be read as an index; keep them 0
        buf = np.zeros(2 * GUARD + flat.size + off, np.int32)
    else:
        buf = np.full(2 * GUARD + flat.size + off, np.nan, np.float32)
    buf[GUARD + off:GUARD + off + flat.size] = flat
    return buf, GUARD + off


def out_buffer(n):
    """a NaN-filled output of n floats between two NaN guards: (buffer, start)"""
    return np.full(2 * GUARD + max(n, 4), np.nan, np.float32), GUARD


def unpack_out(buf, start, shape, what):
    """the output after the call; the guards must still be NaN"""
    n = int(np.prod(shape))
    if not (np.isnan(buf[:start]).all() and np.isnan(buf[start + n:]).all()):
        raise AssertionError("%s: wrote outside the output (a guard is no longer NaN)" % what)
    return buf[start:start + n].reshape(shape)


def untouched(buf, what):
    if not np.isnan(buf).all():
        raise AssertionError("%s: a refused call wrote %d floats of the output" % (what, int((~np.isnan(buf)).sum())))


# -------------------------------------------------------------------------------------------------------- comparators
def _where(bad):
    ij = np.argwhere(bad)
    return "%d elements, first at %s, last at %s" % (len(ij), tuple(ij[0]), tuple(ij[-1]))


def compare(got, r64, scale, kind, coeff, what):
    """exact: got == ref64 element for element; real: |got - ref64| <= coeff * scale.  Returns the worst error as a
    fraction of the bound (0 for exact data).  A NaN (an element never written, or read from a guard) fails both."""
    if got.shape != r64.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, got.shape, r64.shape))
    g = got.astype(np.float64)
    if kind == "exact":
        bad = ~(g == r64)
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s: not exact on integer operands: %s (got %r, want %r)" % (what, _where(bad), got[i], r64[i]))
        return 0.0
    bound = coeff * scale
    err = np.abs(g - r64)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: outside %.3g * scale: %s (got %r, want %r, error %.3g, bound %.3g)"
                             % (what, coeff, _where(bad), got[i], r64[i], err[i], bound[i]))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(a.view(np.int32), b.view(np.int32)):
        raise AssertionError("%s: %s" % (what, _where(a.view(np.int32) != b.view(np.int32)) if a.shape == b.shape else "shapes"))


# -------------------------------------------------------------------------------------------------------- case matrix
def _geo(stride, pad):
    return "s%d-p%d%d" % (stride, pad[0], pad[1])


def _conv(group, what, B, Hi, Wi, Ci, kh, kw, Co, stride=1, pad=(0, 0), **kw_):
    c = Conv(group, "", B, Hi, Wi, Ci, kh, kw, Co, stride, pad, **kw_)
    name = "%s-%s%dx%d-ci%d-co%d-%s-b%d-%dx%d-o%dx%d" % (group, what + "-" if what else "", kh, kw, Ci, Co, _geo(stride, pad),
                                                         B, Hi, Wi, c.Ho, c.Wo)
    if not c.route:
        if c.plain:
            route = "plain 1x1"
        elif Ci < 32:
            route = "four-channel"
        else:
            route = "implicit steady-state" if kh * kw <= 32 else "implicit general"
        c = c._replace(route=route)
    return c._replace(name=name)


def cases_a():
    """the implicit-GEMM k loop (Ci % 32 == 0, at most 32 taps): nt = K / 32 of 1, 2, 3 (1x1 stride 2; with Ci = 96
    advance() crosses a tap every third tile), 9..32 tiles with square, 1 x n, n x 1 and 32-tap filters (bit 31)"""
    out = [_conv("a", "", 2, 7, 7, Ci, 1, 1, 64, 2) for Ci in (32, 64, 96)]
    out += [_conv("a", "", 2, 7, 6, Ci, 3, 3, 64, 1, (1, 1)) for Ci in (32, 64)]
    out += [_conv("a", "", 2, 7, 6, 32, 1, 3, 64, 1, (0, 1)), _conv("a", "", 2, 7, 6, 32, 3, 1, 64, 1, (1, 0)),
            _conv("a", "", 2, 7, 6, 32, 2, 2, 64), _conv("a", "", 3, 5, 3, 96, 2, 2, 64, 1, (1, 0)),
            _conv("a", "", 2, 7, 6, 32, 5, 5, 64, 1, (2, 2)), _conv("a", "", 2, 7, 9, 32, 4, 8, 64, 1, (1, 3)),
            _conv("a", "", 2, 6, 9, 32, 4, 8, 64, 1, (3, 7))]
    return out


def cases_b():
    """the general loop behind the implicit GEMM: more than 32 taps with Ci = 32"""
    return [_conv("b", "", 2, 9, 8, 32, 6, 6, 64, 1, (2, 2)), _conv("b", "", 2, 13, 12, 32, 7, 7, 64, 2, (3, 3)),
            _conv("b", "", 2, 5, 13, 32, 3, 11, 64, 1, (1, 5))]


def cases_c():
    """four-channel pixels (the per-lane tap route): conv1's [7, 8, 4] filter with a zero eighth column on an image whose
    last column lies under the eighth tap of a window; 1 x 8 (K = 32, one k tile); 2 x 4"""
    return [_conv("c", "conv1", 2, 12, 13, 4, 7, 8, 64, 2, (3, 3), out=(6, 7), zero_last_column=True),
            _conv("c", "conv1", 2, 13, 12, 4, 7, 8, 64, 2, (3, 3), out=(7, 6), zero_last_column=True),
            _conv("c", "", 2, 5, 9, 4, 1, 8, 64, 1, (0, 3)), _conv("c", "", 2, 5, 9, 4, 2, 4, 64, 1, (0, 1))]


D_PADS = ((0, 0), (1, 1), (2, 0), (0, 1))
D_FILTERS = ((3, 3, 32), (6, 6, 32), (7, 8, 4))      # one filter of A, B and C


def geometries(kh, kw, full_cross):
    """(stride, pad, Hi, Wi, out) of group D for a filter: pads x strides 1, 2, 3 x an odd x even and an even x odd image,
    with the full extent and with Ho, Wo one less (where the full extent is above 1)"""
    out = []
    for n, (pad, stride) in enumerate(itertools.product(D_PADS, (1, 2, 3))):
        for m, (Hi, Wi) in enumerate(((9, 8), (10, 11))):
            Ho, Wo = full_extent(Hi, kh, stride, pad[0]), full_extent(Wi, kw, stride, pad[1])
            for less in (0, 1):
                if not full_cross and (n + m + less) % 2:
                    continue
                o = (max(Ho - less, 1), max(Wo - less, 1))
                if less and o == (Ho, Wo):
                    continue
                out.append((stride, pad, Hi, Wi, o if less else None))
    return out


def cases_d():
    """geometry: every pad of D_PADS (top != left included) x stride 1, 2, 3 x odd and even images x the full extent and
    one less, on one filter of each of A, B and C; a padding of 4 on a 3x3, where whole windows lie outside the image"""
    out = []
    for kh, kw, Ci in D_FILTERS:
        for stride, pad, Hi, Wi, o in geometries(kh, kw, full_cross=(kh, kw) == (3, 3)):
            out.append(_conv("d", "", 2, Hi, Wi, Ci, kh, kw, 64, stride, pad, out=o))
    out.append(_conv("d", "", 2, 7, 6, 32, 3, 3, 64, 1, (4, 4)))
    out.append(_conv("d", "", 2, 7, 6, 32, 3, 3, 64, 2, (4, 4)))
    return out


E_SHAPES = {1: (1, 1, 1), 63: (3, 3, 7), 64: (4, 4, 4), 65: (5, 1, 13), 129: (3, 1, 43)}     # M: (B, Hi, Wi)


def cases_e():
    """tile edges: M = B Ho Wo of 1, 63, 64, 65, 129 with several images inside one tile, Co of 4, 60, 64, 68, 132, on
    the steady-state route (3x3 'same') and the four-channel route (2x4)"""
    out = []
    for M, (B, Hi, Wi) in E_SHAPES.items():
        out.append(_conv("e", "M%d" % M, B, Hi, Wi, 32, 3, 3, 64, 1, (1, 1)))
        out.append(_conv("e", "M%d" % M, B, Hi, Wi, 4, 2, 4, 64, 1, (0, 1), out=(Hi, Wi)))
    B, Hi, Wi = E_SHAPES[65]
    for Co in (4, 60, 68, 132):
        out.append(_conv("e", "M65", B, Hi, Wi, 32, 3, 3, Co, 1, (1, 1)))
        out.append(_conv("e", "M65", B, Hi, Wi, 4, 2, 4, Co, 1, (0, 1), out=(Hi, Wi)))
    return out


EPILOGUES = tuple(itertools.product((False, True), (False, True), (False, True), (0, 1)))    # scale, shift, residual, relu


def _epi(c, tag, route, **kw):
    out = []
    for scale, shift, residual, relu in EPILOGUES:
        what = "%s-%s%s%s%s" % (tag, "S" if scale else "s", "H" if shift else "h", "R" if residual else "r", "+" if relu else "-")
        out.append(c._replace(name=c.name.replace("f-", "f-%s-" % what, 1), scale=scale, shift=shift, residual=residual,
                              relu=relu, route=route, **kw))
    return out


def cases_f_by_route():
    """{tag: cases}: all eight NULL / non-NULL combinations of scale, shift and residual x relu on every forward route"""
    one = _conv("f", "", 2, 5, 5, 64, 1, 1, 64)
    out = {"implicit": _epi(_conv("f", "", 2, 5, 5, 32, 3, 3, 64, 1, (1, 1)), "implicit", "implicit steady-state"),
           "cfg3": _epi(one, "cfg3", "plain 1x1 cfg 3"),
           "cfg16": _epi(one, "cfg16", "plain 1x1 cfg 16", gcfg=16),
           "cfg20": _epi(one, "cfg20", "plain 1x1 cfg 20", gcfg=20), "shortk": [], "shortk-off": []}
    for Ci in (128, 256):
        wide = _conv("f", "", 2, 5, 5, Ci, 1, 1, 2 * Ci)
        out["shortk"] += _epi(wide, "shortk", "short-K 1x1")
        out["shortk-off"] += _epi(wide, "shortk-off", "plain 1x1 cfg 3", shortk=1)
    return out


def cases_f():
    return [c for cs in cases_f_by_route().values() for c in cs]


def cases_g():
    """vqa_conv_set_config 0..3 over groups A, C and E"""
    out = []
    for cfg in range(4):
        for c in cases_a() + cases_c() + cases_e():
            out.append(c._replace(group="g", name="g-ccfg%d-%s" % (cfg, c.name), ccfg=cfg, route="%s, tile config %d" % (c.route, cfg)))
    return out


def cases_h():
    """the 1x1 route with Ci = 6, Co = 10: no multiple of 4 anywhere.  Outcome: accepted and right -- the plain route
    hands shapes the buffer-load loaders cannot serve to the GEMM's edge loader (launch_edge), as vqa_gemm_f32 does"""
    return [_conv("h", "", 2, 5, 5, 6, 1, 1, 10, route="plain 1x1, edge loader"),
            _conv("h", "shift-only", 2, 5, 5, 6, 1, 1, 10, route="plain 1x1, edge loader", scale=False, residual=False, relu=0),
            _conv("h", "x+1", 2, 5, 5, 8, 1, 1, 12, route="plain 1x1, edge loader", x_off=1)]


def cases_i():
    """refusals: the code of the header, y still NaN"""
    base = dict(kinds=("exact",), route="refused")
    return [_conv("i", "ci48", 2, 5, 5, 48, 3, 3, 64, 1, (1, 1), expect=ERR_ALIGN, **base),
            _conv("i", "K36", 2, 5, 5, 4, 3, 3, 64, 1, (1, 1), expect=ERR_ALIGN, **base),
            _conv("i", "co6", 2, 5, 5, 32, 3, 3, 6, 1, (1, 1), expect=ERR_UNSUPPORTED, **base),
            _conv("i", "x+1", 2, 5, 5, 32, 3, 3, 64, 1, (1, 1), expect=ERR_ALIGN, x_off=1, **base),
            _conv("i", "null-x", 2, 5, 5, 32, 3, 3, 64, 1, (1, 1), expect=ERR_ARG, null="x", **base),
            _conv("i", "null-w", 2, 5, 5, 32, 3, 3, 64, 1, (1, 1), expect=ERR_ARG, null="w", **base),
            _conv("i", "null-y", 2, 5, 5, 32, 3, 3, 64, 1, (1, 1), expect=ERR_ARG, null="y", **base),
            _conv("i", "null-x-1x1", 2, 5, 5, 32, 1, 1, 64, expect=ERR_ARG, null="x", **base)]


# non-positive sizes of vqa_conv2d_nhwc: the argument (by position in the header) that is zeroed or negated
I_NONPOSITIVE = ("B", "Hi", "Wi", "Ci", "kh", "kw", "Co", "stride", "Ho", "Wo")

J_FILTERS = (("pw", 1, 1, 1, 8), ("1x1s2", 1, 1, 2, 8), ("3x3", 3, 3, 1, 8), ("1x3", 1, 3, 1, 8), ("7x7s2", 7, 7, 2, 4))


def _bwd(what, B, Hi, Wi, Ci, kh, kw, Co, stride=1, pad=(0, 0), **kw_):
    c = Bwd("j", "", B, Hi, Wi, Ci, kh, kw, Co, stride, pad, **kw_)
    name = "j-%s%dx%d-ci%d-co%d-%s-b%d-%dx%d-o%dx%d" % (what + "-" if what else "", kh, kw, Ci, Co, _geo(stride, pad), B, Hi, Wi,
                                                       c.Ho, c.Wo)
    n = -(-c.B // c.chunks)
    route = ("pointwise" if c.pointwise else "im2col") + (", one chunk" if n == 1 else ", %d chunks%s" % (n, " (ragged)" if c.B % c.chunks else ""))
    return c._replace(name=name, route=route)


def cases_j_geometry():
    """every filter of J_FILTERS (the filter's own stride replaced by the geometry's) under D's geometries, the padding
    of 4, and VALID stride 2 on an image whose last row and column belong to no window (dx exactly 0 there)"""
    out = []
    for tag, kh, kw, s0, Ci in J_FILTERS:
        if tag == "1x1s2":       # the same filter as "pw": its geometries differ only by the default stride
            continue
        for stride, pad, Hi, Wi, o in geometries(kh, kw, full_cross=False):
            if full_extent(Hi, kh, stride, pad[0]) < 1 or full_extent(Wi, kw, stride, pad[1]) < 1:
                continue
            out.append(_bwd("", 2, Hi, Wi, Ci, kh, kw, 16, stride, pad, out=o))
    out.append(_bwd("", 2, 7, 6, 8, 3, 3, 16, 1, (4, 4)))
    for tag, kh, kw, s0, Ci in J_FILTERS:
        Hi, Wi = (kh + 2 * 2 + 1, kw + 2 * 2 + 1)        # (Hi - kh) odd: VALID stride 2 leaves the last row and column over
        out.append(_bwd("valid-" + tag, 2, Hi, Wi, Ci, kh, kw, 16, 2 if tag != "pw" else s0))
        out.append(_bwd("valid3-" + tag, 2, kh + 4, kw + 4, Ci, kh, kw, 16, 3))    # rows 0..kh+2 of kh+4 are covered
    return out


def cases_j_edges():
    """M = B Ho Wo of 1, 3, 5 (dshift's four row groups with fewer than four rows) and Co of 4, 64, 68 (dshift's 64-channel
    blocks) on every filter"""
    out = []
    for tag, kh, kw, stride, Ci in J_FILTERS:
        for M in (1, 3, 5):      # M images of one output pixel: Hi = kh, Wi = kw
            out.append(_bwd("M%d-%s" % (M, tag), M, kh, kw, Ci, kh, kw, 64, stride))
        for Co in (4, 64, 68):
            out.append(_bwd(tag, 2, kh + 3, kw + 2, Ci, kh, kw, Co, stride, (kh // 2, kw // 2)))
    return out


def cases_j_nulls():
    """each output NULL in turn and only one output at a time, scale NULL, relu = 0 with y = NULL and with a y that must
    be ignored, planted zeros, on the im2col and the pointwise route"""
    out = []
    for tag, kh, kw, pad in (("3x3", 3, 3, (1, 1)), ("pw", 1, 1, (0, 0))):
        base = dict(B=2, Hi=5, Wi=4, Ci=8, kh=kh, kw=kw, Co=12, pad=pad)
        names = ("dx", "dw", "dshift", "dresidual")
        for skip in names:
            out.append(_bwd("no-%s-%s" % (skip, tag), outs=tuple(n for n in names if n != skip), **base))
            out.append(_bwd("only-%s-%s" % (skip, tag), outs=(skip,), **base))
        out.append(_bwd("no-scale-" + tag, scale=False, **base))
        out.append(_bwd("linear-ynull-" + tag, relu=0, y_null=True, **base))
        out.append(_bwd("linear-" + tag, relu=0, **base))
        out.append(_bwd("planted-" + tag, plant=True, **base))
    return out


def cases_j_chunks():
    """B = 5 under the workspace of chunk_images 5, 2 and 1: one chunk, chunks of 2, 2, 1 (ragged) and five chunks"""
    out = []
    for tag, kh, kw, pad in (("3x3", 3, 3, (1, 1)), ("pw", 1, 1, (0, 0))):
        out.append([_bwd("chunk%d-%s" % (ch, tag), 5, 5, 4, 8, kh, kw, 12, 1, pad, chunk=ch) for ch in (5, 2, 1)])
    return out


def cases_j_refusals():
    base = dict(kinds=("exact",))
    return [_bwd("ws-short", 5, 5, 4, 8, 3, 3, 12, 1, (1, 1), chunk=1, ws_short=1, expect=ERR_WORKSPACE, **base),
            _bwd("ws-short-pw", 5, 5, 4, 8, 1, 1, 12, chunk=1, ws_short=1, expect=ERR_WORKSPACE, **base),
            _bwd("ci6", 2, 5, 4, 6, 3, 3, 12, 1, (1, 1), expect=ERR_ALIGN, **base),
            _bwd("co6", 2, 5, 4, 8, 3, 3, 6, 1, (1, 1), expect=ERR_ALIGN, **base)]


def cases_j():
    return cases_j_geometry() + cases_j_edges() + cases_j_nulls() + [c for g in cases_j_chunks() for c in g] + cases_j_refusals()


CROP_SIZES = ((1, 1), (1, 3), (3, 1), (5, 5), (3, 2))
CROP_MAPS = ((5, 5), (1, 5), (5, 1), (9, 5))
CROP_CHANNELS = (1, 4, 255, 256, 257, 513)


def cases_k():
    """crop and resize: every crop size on every map size with C = 4, every channel count around the 256-lane loop
    stride on the 9 x 5 map with a 3 x 2 crop, n_boxes = 0"""
    out = [Crop("k-%dx%d-map%dx%d-c4" % (ch, cw, H, W), 3, H, W, 4, ch, cw) for (ch, cw) in CROP_SIZES for (H, W) in CROP_MAPS]
    out += [Crop("k-3x2-map9x5-c%d-b2" % C, 2, 9, 5, C, 3, 2) for C in CROP_CHANNELS]
    out += [Crop("k-5x5-map5x5-c257-b1", 1, 5, 5, 257, 5, 5), Crop("k-empty", 2, 5, 5, 4, 3, 3, boxes="none")]
    return out


def cases_l():
    """pool, subsample, pad: Hi, Wi of 1, 2, 3, 8, 9, C of 4, 12, 64, factors 1, 2, 3, an all-negative pool input, C = 6
    refused"""
    out = []
    sizes = (1, 2, 3, 8, 9)
    for n, (Hi, Wi) in enumerate(itertools.product(sizes, sizes)):
        C = (4, 12, 64)[n % 3]
        out.append(Pool("l-maxpool-%dx%d-c%d" % (Hi, Wi, C), "maxpool", 2, Hi, Wi, C))
        out.append(Pool("l-subsample%d-%dx%d-c%d" % (n % 3 + 1, Hi, Wi, C), "subsample", 2, Hi, Wi, C, factor=n % 3 + 1))
    for C in (4, 12, 64):
        for f in (1, 2, 3):
            out.append(Pool("l-subsample%d-9x8-c%d-b3" % (f, C), "subsample", 3, 9, 8, C, factor=f))
        out.append(Pool("l-maxpool-negative-9x8-c%d" % C, "maxpool", 3, 9, 8, C, negative=True))
        out.append(Pool("l-maxpool-negative-2x1-c%d" % C, "maxpool", 2, 2, 1, C, negative=True))
    for Hi, Wi in ((1, 1), (3, 2), (9, 8), (13, 13)):
        out.append(Pool("l-pad-%dx%d" % (Hi, Wi), "pad", 2, Hi, Wi, 4))
    out += [Pool("l-maxpool-c6", "maxpool", 2, 3, 3, 6, expect=ERR_ALIGN),
            Pool("l-subsample-c6", "subsample", 2, 3, 3, 6, factor=2, expect=ERR_ALIGN)]
    return out


def matrix():
    """every case of tests/test_gpu_conv_f64.py"""
    return (cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_f() + cases_g() + cases_h() + cases_i() +
            cases_j() + cases_k() + cases_l())
