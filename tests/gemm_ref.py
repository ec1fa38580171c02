"""Float64 reference of the f32 MFMA GEMM of include/vqa_hot.h (vqa_gemm_f32, vqa_gemm_f32_ex, vqa_gemm_f32_gather;
csrc/gemm_f32.hip), the data, the guarded buffers and the comparators of its op-level tests, and the case matrix that
crosses every route of the dispatcher with every edge of its loops.

ref(case, kind) evaluates the header's contract in float64 numpy, C = op(A) @ op(B) (+ bias) (+ D), the gather form
with its rows built through idx under the clamp of vqa_gather_features, and returns beside it the magnitude sum
scale = |op(A)| @ |op(B)| + |bias| + |D| that a rounding error is proportional to.

Two kinds of data for every case:
  exact   A, B, bias and D are independent integers in [-3, 3] stored as float32.  Every partial sum of every
          summation order is an integer of magnitude <= 9 K + 6 < 2^24, so every order is exact and the comparator is
          array_equal with the float64 value: zero tolerance, whatever the tile, the k grouping or the slab count.
  real    standard normal operands, judged element by element:
              |got - ref64| <= min(RT, (K + S + 6) 2^-24) * scale
          (K + S + 6) 2^-24 is the worst-case bound of ANY float32 summation of K exact-product terms (one rounding per
          fused multiply-add), the S slab sums of the requested split, up to four in-block k groups, bias and D.  RT is
          measured, not chosen: the float32 evaluation of this reference on the CPU in the two extreme orders a kernel
          can take (sequential over k; 8-wide chunks summed, then combined), worst |ref32 - ref64| / scale over every
          `real` case of the matrix, times 8 -- the margin the project's other references give a difference in
          summation order.  tests/test_gemm_reference.py measures it, holds this table to the live measurement and
          holds both float32 evaluations inside the bound (at most 1/8 of RT by construction).

  float32 worst   RT = 8x    at
  4.00e-07        3.2e-06    a-plain-cfg0-NT-300x200x36, sequential order (NT 300 x 200 x 36 without bias and D: 6.7 U,
                             the tail of 60 000 sequential 36-term sums whose scale has neither bias nor D in it)
RT is 53.7 U, so the derived cap (K + S + 6) U is the smaller term up to K = 46 at S = 1 and RT is above.

Buffers: every operand with a leading dimension above its width carries NaN in the padding, so a loader that reads
past a row's K, M or N shows as NaN in C; an operand offset by one float starts 4 bytes past a 16-byte boundary.  C sits
in a NaN-filled buffer between two NaN guards: its own padding columns N..ldc-1 and the guards must still be NaN after
the call (a padded addend aliased to C holds the addend's values in the columns < N instead).  The gather form's
gathered_out is guarded the same way.  No loader of csrc/gemm_f32.hip reads padding and discards it: the fast loaders
substitute an out-of-range buffer offset for every float4 outside the operand (K % 4 == 0 and the row width % 4 == 0 keep a
float4 wholly in or out), the steady-state loop clamps rows past M / N onto valid rows, and the edge loader counts the
valid elements of every float4.  So NaN is everywhere.

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import typing
import zlib

import numpy as np

U = 2.0 ** -24                  # unit roundoff of float32
RT = 3.2e-06                    # 8x MEASURED_F32
MEASURED_F32 = 4.00e-07
MEASURED_AT = "a-plain-cfg0-NT-300x200x36 (seq)"
OK, ERR_ARG, ERR_ALIGN, ERR_LAUNCH, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -3, -4, -5
GUARD = 64                      # floats of NaN on either side of an output (a multiple of 16 bytes)

LAYOUTS = {"NN": (0, 0), "NT": (0, 1), "TN": (1, 0)}
LAYOUT_OF = {v: k for k, v in LAYOUTS.items()}

# launch_by_id of csrc/gemm_f32.hip: cfg -> (BM, BN, WGK in-block k groups, BK k-tile depth, two-tile prefetch, threads);
# tests/test_gemm_reference.py holds this table to the source
CFG = {
    0: (128, 128, 1, 16, 0, 256), 1: (128, 128, 1, 32, 0, 256), 2: (64, 64, 1, 16, 0, 256), 3: (64, 64, 1, 32, 0, 256),
    4: (64, 64, 1, 64, 0, 256), 5: (128, 64, 1, 32, 0, 256), 6: (64, 128, 1, 32, 0, 256), 7: (64, 32, 2, 64, 0, 256),
    8: (32, 32, 4, 64, 0, 256), 9: (32, 64, 2, 64, 0, 256), 10: (64, 64, 1, 64, 1, 256), 11: (64, 32, 2, 64, 1, 256),
    12: (64, 64, 1, 32, 1, 256), 13: (64, 32, 2, 32, 1, 256), 14: (128, 32, 1, 64, 1, 256), 15: (128, 64, 1, 32, 1, 256),
    16: (128, 128, 1, 32, 0, 512), 17: (128, 128, 1, 32, 0, 512), 18: (256, 64, 1, 32, 0, 512), 19: (128, 128, 1, 16, 0, 512),
    20: (128, 64, 1, 32, 0, 512), 21: (64, 128, 1, 32, 0, 512), 22: (128, 64, 1, 16, 0, 512), 23: (64, 32, 4, 32, 1, 512),
}
NUM_CFG = 24
# the other id namespaces of csrc/gemm_tiles.h, mirrored by hand like CFG and held to the source by the same test.
# GRU-step id (vqa_gemm_set_gru_config) -> (tile of the 2H-wide gate GEMM, tile of the H-wide GEMMs), tiles in CFG's form
_GRU_32 = (32, 32, 4, 32, 1, 256)
GRU_CFG = {4: (CFG[4], CFG[4]), 7: (CFG[7], CFG[7]), 8: (CFG[8], CFG[8]), 9: (CFG[9], CFG[9]), 10: (CFG[10], CFG[10]),
           11: (CFG[11], CFG[11]), 12: (CFG[12], CFG[12]), 13: (CFG[13], CFG[13]), 16: (_GRU_32, _GRU_32),
           17: (CFG[23], CFG[23]), 18: ((64, 64, 4, 64, 1, 1024), (64, 32, 8, 64, 1, 1024)), 20: (CFG[20], CFG[20]),
           21: (CFG[21], CFG[21])}
GRU_STREAMED, GRU_STREAMED_FALLBACK = 30, 16      # the register-streamed step kernels and the id their refusals run under
CONV_CFG = {0: 3, 1: 20, 2: 21, 3: 16}            # conv id (vqa_conv_set_config) -> plain id of its tile
TALL_CFGS = (20, 21)                              # vqa_gemm_set_tall_config; the row-gathered product takes the same tile
EDGE_CFG = 2                                      # plain id of the tile behind the guarded loaders
# one configuration per class of kernel (the scalar-epilogue and the persistent-walk cases run these)
CLASS_CFGS = (2, 7, 8, 12, 16, 20, 23)
WGK1_CLASS_CFGS = (2, 12, 16, 20)
SPLIT_PAIRS = ((128, 2), (132, 2), (200, 4), (260, 3), (448, 7), (1028, 16), (64, 4))
M0, N0 = 300, 200               # two tiles each way with a ragged last one for every BM, BN up to 256; both % 4 == 0


def class_of(cfg):
    """the kernel class of a configuration (what the GPU test's worst-error table is keyed by)"""
    BM, BN, wgk, BK, deep, nt = CFG[cfg]
    name = "512-thread" if nt == 512 else "4-wave"
    if deep:
        name += " two-tile-prefetch"
    return name + " WGK %d" % wgk


def ks_for(BK):
    """1..7 k tiles with and without a partial last tile: every rem of the two-tile loop, both parities of the other
    (6 BK beside the issue's list, which has no K of exactly six tiles)"""
    return sorted({4, BK - 4, BK, BK + 4, 2 * BK, 2 * BK + 4, 3 * BK, 4 * BK - 4, 4 * BK, 5 * BK, 6 * BK, 6 * BK + 4, 7 * BK})


# -------------------------------------------------------------------------------------------------------------- cases
class Case(typing.NamedTuple):
    group: str
    name: str
    cfg: int                     # forced with vqa_gemm_set_config; -1: the automatic choice
    tA: int
    tB: int
    M: int
    N: int
    K: int
    split: int = 1               # the split_k argument (0: automatic)
    bias: bool = True
    D: str = "own"               # "own": a buffer of its own, "none": NULL, "alias": D == C (in-place accumulate)
    pad: tuple = (0, 0, 0, 0)    # lda, ldb, ldc, ldd beyond the stored width
    off: tuple = (0, 0, 0, 0, 0)  # A, B, C, bias, D: floats past a 16-byte boundary
    ws: typing.Optional[int] = 0  # workspace floats relative to what the split needs (-1: one short); None: no workspace
    max_blocks: int = 0
    order: int = -1              # vqa_gemm_set_order
    entry: str = "ex"            # "ex": vqa_gemm_f32_ex(..., max_blocks); "f32": vqa_gemm_set_max_blocks + vqa_gemm_f32
    shortk: int = -1             # vqa_gemm_shortk_set_mode
    expect: int = OK
    kinds: tuple = ("exact", "real")
    auto: tuple = ()             # (cfg, split) the automatic choice must make (group f and the automatic edge split)

    def id(self):
        return self.name

    @property
    def layout(self):
        return LAYOUT_OF[(self.tA, self.tB)]

    @property
    def S(self):
        """the requested split (the automatic one where split_k == 0)"""
        return self.split if self.split > 0 else (self.auto[1] if self.auto else 1)


class GatherCase(typing.NamedTuple):
    name: str
    tall: int                    # vqa_gemm_set_tall_config: 20 (128 x 64 tiles) or 21 (64 x 128)
    B: int                       # samples in the batch
    R: int                       # regions (rows) per sample
    N: int
    K: int
    ns: int                      # samples in the table
    gout: str = "none"           # gathered_out: "none", "dense", "padded" (ldg = K + 4), "offset" (one float off)
    bias: bool = True
    pad: tuple = (0, 0, 0)       # lda, ldb, ldc beyond the width
    expect: int = OK
    kinds: tuple = ("exact", "real")

    def id(self):
        return self.name

    @property
    def M(self):
        return self.B * self.R


def geometry(c):
    """{operand: (rows, width, ld, offset)} as stored"""
    ra, wa = (c.K, c.M) if c.tA else (c.M, c.K)
    rb, wb = (c.N, c.K) if c.tB else (c.K, c.N)
    g = {"A": (ra, wa, wa + c.pad[0], c.off[0]), "B": (rb, wb, wb + c.pad[1], c.off[1]),
         "C": (c.M, c.N, c.N + c.pad[2], c.off[2]), "bias": (1, c.N, c.N, c.off[3])}
    g["D"] = g["C"] if c.D == "alias" else (c.M, c.N, c.N + c.pad[3], c.off[4])
    return g


def fast_ok(c):
    """fast_ok() of the dispatcher: the buffer-load loaders serve the case (else launch_edge does)"""
    g = geometry(c)
    vec = all(g[x][2] % 4 == 0 and g[x][3] % 4 == 0 for x in "AB")
    return vec and c.K >= 4 and c.K % 4 == 0 and (not c.tA or c.M % 4 == 0) and (c.tB or c.N % 4 == 0)


def slabs(c):
    """the slab count a split request collapses to (vqa_gemm_f32_ex)"""
    s = c.S
    if s <= 1 or c.N % 4 != 0 or c.ws is None or c.K == 0:
        return 1
    kps = -(-(-(-c.K // s)) // 64) * 64
    return -(-c.K // kps)


def vec_epi(c):
    """the 16-byte epilogue serves the case (else the 16-dword one does)"""
    g = geometry(c)
    al = lambda x, ld=True: (not ld or g[x][2] % 4 == 0) and g[x][3] % 4 == 0
    if c.N % 4 != 0 or (c.bias and not al("bias", False)) or (c.D != "none" and not al("D")):
        return False
    return True if slabs(c) > 1 else al("C")


def k_tiles(c):
    return -(-c.K // CFG[c.cfg][3])


def tiles(c):
    BM, BN = (64, 64) if (c.cfg < 0 or not fast_ok(c)) else CFG[c.cfg][:2]
    return -(-c.M // BM) * -(-c.N // BN) * slabs(c)


def choose(tA, tB, M, N, K, split_k=0, tall=20):
    """choose() of csrc/gemm_f32.hip under its default environment: (cfg, split)"""
    cd = lambda a, b: -(-a // b)
    if tA:
        mid = K < 20000 and cd(M, 128) * cd(N, 128) <= 128
        cfg = (20 if K <= 4096 else (20 if mid else 19)) if M * N >= (1 << 20) else 3
        target = 512
    elif M >= 2048:
        cfg = (tall if K >= 2048 else 22) if N >= 512 else 13
        target = 256
        if N >= 512 and cd(M, 128) * cd(N, 64) < 1024:
            cfg = 12
    else:
        cfg, target = (13 if (not tB and N > 2048) else 23), 256
    want = 0
    if not tA and tB and M >= 4096 and N <= 320 and K >= 2048:
        cfg, want = 3, 4
    elif tA and M <= 320 and N >= 2048 and K >= 4096:
        cfg, want = 21, 4
    blocks = cd(M, CFG[cfg][0]) * cd(N, CFG[cfg][1])
    split = split_k
    if split <= 0:
        split = 1
        if N % 4 == 0:
            if want:
                split = want
            else:
                while blocks * split < target and K // (split * 2) >= 256 and split < 16:
                    split *= 2
    return cfg, split


def takes_shortk(c):
    """the hand-off of vqa_gemm_f32_ex to gemm_shortk.hip under the default mode (dense or 16-byte aligned operands)"""
    return (not c.tA and not c.tB and c.split <= 1 and c.max_blocks == 0 and c.cfg < 0 and c.shortk != 0 and
            c.M >= 1024 and c.K <= 304 and c.K % 4 == 0 and c.N % 32 == 0 and not (c.K > 256 and c.D != "none") and
            all(x % 4 == 0 for x in c.pad) and all(x % 4 == 0 for x in c.off))


# --------------------------------------------------------------------------------------------------------------- data
_DATA: dict = {}
_REF: dict = {}
_BIG = 1 << 22                   # operands above this many elements are not kept


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _draw(rng, kind, *shape):
    if kind == "exact":
        return rng.randint(-3, 4, size=shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def operands(c, kind):
    """the logical operands {A [M,K], B [K,N], bias [N], D [M,N]} (float32) of a Case; cases of one shape and layout
    share them, so the reference of a shape is taken once"""
    key = (kind, c.tA, c.tB, c.M, c.N, c.K)
    if key not in _DATA:
        rng = _rng(*key)
        d = {"A": _draw(rng, kind, c.M, c.K), "B": _draw(rng, kind, c.K, c.N), "bias": _draw(rng, kind, c.N),
             "D": _draw(rng, kind, c.M, c.N)}
        if c.M * c.K + c.K * c.N > _BIG:
            return d
        _DATA[key] = d
    return _DATA[key]


def _product(A, B, bias, D, dtype=np.float64):
    out = A.astype(dtype) @ B.astype(dtype)
    if bias is not None:
        out = out + bias.astype(dtype)[None, :]
    if D is not None:
        out = out + D.astype(dtype)
    return out


def ref(c, kind, ops=None):
    """(ref64 [M,N], scale [M,N]) of a Case or a GatherCase"""
    if isinstance(c, GatherCase):
        d = ops if ops is not None else gather_operands(c, kind)
        A = gathered_rows(d["table"], d["idx"], c.R, c.ns)
        bias = d["bias"] if c.bias else None
        return _product(A, d["B"], bias, None), _product(np.abs(A), np.abs(d["B"]), None if bias is None else np.abs(bias), None)
    key = (kind, c.tA, c.tB, c.M, c.N, c.K, c.bias, c.D != "none")
    if key in _REF:
        return _REF[key]
    d = ops if ops is not None else operands(c, kind)
    bias, D = (d["bias"] if c.bias else None), (d["D"] if c.D != "none" else None)
    r = _product(d["A"], d["B"], bias, D)
    if kind == "exact":          # |ref| <= scale <= 9 K + 6: the scale is not used by the exact comparator
        s = np.abs(r)
    else:
        s = _product(np.abs(d["A"]), np.abs(d["B"]), None if bias is None else np.abs(bias), None if D is None else np.abs(D))
    if c.M * c.N <= _BIG // 4:
        _REF[key] = (r, s)
    return r, s


def ref32(c, kind, order, ops=None):
    """the float32 evaluation of the contract in one of the two extreme orders a kernel can take: "seq" adds the K
    products one by one, "chunk8" sums every 8 consecutive k first and then adds the chunks; bias, then D, last"""
    if isinstance(c, GatherCase):
        d = ops if ops is not None else gather_operands(c, kind)
        A, B, bias, D = gathered_rows(d["table"], d["idx"], c.R, c.ns), d["B"], (d["bias"] if c.bias else None), None
    else:
        d = ops if ops is not None else operands(c, kind)
        A, B, bias, D = d["A"], d["B"], (d["bias"] if c.bias else None), (d["D"] if c.D != "none" else None)
    M, K = A.shape
    acc = np.zeros((M, B.shape[1]), np.float32)
    if order == "seq":
        for k in range(K):
            acc += A[:, k, None] * B[k, None, :]
    else:
        for k0 in range(0, K, 8):
            part = np.zeros_like(acc)
            for k in range(k0, min(K, k0 + 8)):
                part += A[:, k, None] * B[k, None, :]
            acc += part
    if bias is not None:
        acc += bias[None, :]
    if D is not None:
        acc += D
    return acc


def gather_operands(g, kind):
    """{table [ns*R, K], idx int64 [B] with duplicates, -1 and ns + 5, B [K,N], bias [N]}"""
    key = (kind, "gather", g.B, g.R, g.N, g.K, g.ns)
    if key not in _DATA:
        rng = _rng(*key)
        idx = rng.randint(0, g.ns, size=g.B).astype(np.int64)
        idx[0] = -1                                       # clamps to 0
        idx[-1] = g.ns + 5                                # clamps to ns - 1
        if g.B > 3:
            idx[2] = idx[1]                               # a duplicate
        elif g.B == 3:
            idx[1] = 0                                    # a duplicate of what -1 clamps to
        _DATA[key] = {"table": _draw(rng, kind, g.ns * g.R, g.K), "idx": idx, "B": _draw(rng, kind, g.K, g.N),
                      "bias": _draw(rng, kind, g.N)}
    return _DATA[key]


def gathered_rows(table, idx, R, ns):
    """row m of the left operand is row clamp(idx[m // R], 0, ns - 1) * R + m % R of the table"""
    src = np.clip(idx, 0, ns - 1)
    return table.reshape(ns, R, -1)[src].reshape(len(idx) * R, -1)


# ------------------------------------------------------------------------------------------------------------ buffers
def pack(arr, ld, off=0):
    """arr [rows, width] in a NaN-filled flat float32 buffer: element (r, j) at off + r * ld + j.  The buffer's own
    start is taken to be 16-byte aligned, so `off` floats is the misalignment.  Returns the buffer."""
    arr = np.atleast_2d(arr)
    rows, width = arr.shape
    buf = np.full(max(off + rows * ld, 4), np.nan, np.float32)
    if rows * width:
        buf[off:off + rows * ld].reshape(rows, ld)[:, :width] = arr
    return buf


def out_buffer(rows, width, ld, off=0, init=None):
    """a NaN-filled output of `rows` rows of leading dimension ld between two NaN guards; (buffer, start).  `init`
    [rows, width]: what the columns < width hold beforehand (an addend aliased to C)"""
    start = GUARD + off
    buf = np.full(start + rows * ld + GUARD, np.nan, np.float32)
    if init is not None:
        buf[start:start + rows * ld].reshape(rows, ld)[:, :width] = init
    return buf, start


def c_buffer(c, ops):
    _, _, ldc, off = geometry(c)["C"]
    return out_buffer(c.M, c.N, ldc, off, ops["D"] if c.D == "alias" else None)


def unpack_out(buf, start, rows, width, ld, what):
    """the [rows, width] output of a guarded buffer after the call; the guards and the padding columns must be NaN"""
    body = buf[start:start + rows * ld].reshape(rows, ld)
    if not (np.isnan(buf[:start]).all() and np.isnan(buf[start + rows * ld:]).all()):
        raise AssertionError("%s: wrote outside the output (a guard is no longer NaN)" % what)
    if ld > width and not np.isnan(body[:, width:]).all():
        r, j = np.argwhere(~np.isnan(body[:, width:]))[0]
        raise AssertionError("%s: wrote the padding of the output, first at row %d column %d" % (what, r, width + j))
    return body[:, :width]


def untouched(c, buf, start, ops, what):
    """after a refusal: C holds what it held (NaN, or the aliased addend)"""
    want, _ = c_buffer(c, ops)
    if not np.array_equal(buf.view(np.int32), want.view(np.int32)):
        raise AssertionError("%s: C was written by a refused call" % what)


# -------------------------------------------------------------------------------------------------------- comparators
def coefficient(K, S):
    return min(RT, (K + S + 6) * U)


def _where(bad, tile=32):
    ij = np.argwhere(bad)
    (r0, c0), (r1, c1) = ij.min(0), ij.max(0)
    return "%d elements, rows %d..%d, columns %d..%d, first at (%d, %d) = 32x32 sub-tile (%d, %d)" % (
        len(ij), r0, r1, c0, c1, ij[0][0], ij[0][1], ij[0][0] // tile, ij[0][1] // tile)


def compare(got, r64, scale, kind, K, S, what):
    """exact: got == ref64 element for element; real: |got - ref64| <= min(RT, (K + S + 6) U) * scale.  Returns the worst
    error as a fraction of the bound (0 for exact data).  A NaN (an element never written, or a NaN read from an
    operand's padding) fails both."""
    if got.shape != r64.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, got.shape, r64.shape))
    g = got.astype(np.float64)
    if kind == "exact":
        bad = ~(g == r64)
        if bad.any():
            i, j = np.argwhere(bad)[0]
            raise AssertionError("%s: not exact on integer operands: %s (got %r, want %r)" % (what, _where(bad), got[i, j], r64[i, j]))
        return 0.0
    bound = coefficient(K, S) * scale
    err = np.abs(g - r64)
    bad = ~(err <= bound)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("%s: outside %.3g * scale: %s (got %r, want %r, error %.3g, bound %.3g)"
                             % (what, coefficient(K, S), _where(bad), got[i, j], r64[i, j], err[i, j], bound[i, j]))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def same_bits(a, b, what):
    if not np.array_equal(a.view(np.int32), b.view(np.int32)):
        raise AssertionError("%s: %s" % (what, _where(a.view(np.int32) != b.view(np.int32))))


def measure_rt(cases, check=False):
    """(worst |ref32 - ref64| / scale over the `real` cases in both orders, the case and order it came from); check:
    every float32 evaluation is also held to the comparator's bound"""
    worst, at, seen = 0.0, None, set()
    for c in cases:
        if "real" not in c.kinds or c.expect != OK or c.M * c.N == 0:
            continue
        gather = isinstance(c, GatherCase)
        key = (c.B, c.R, c.N, c.K, c.ns, c.bias) if gather else (c.tA, c.tB, c.M, c.N, c.K, c.bias, c.D != "none")
        if key in seen:
            continue
        seen.add(key)
        r64, scale = ref(c, "real")
        nz = scale > 0
        for order in ("seq", "chunk8"):
            r32 = ref32(c, "real", order)
            if check:
                compare(r32, r64, scale, "real", c.K, 1, "%s (%s)" % (c.id(), order))
            e = np.abs(r32.astype(np.float64) - r64)
            assert not e[~nz].any()
            x = float((e[nz] / scale[nz]).max()) if nz.any() else 0.0
            if x > worst:
                worst, at = x, "%s (%s)" % (c.id(), order)
    return worst, at


# -------------------------------------------------------------------------------------------------------- case matrix
def _case(group, what, cfg, layout, M, N, K, **kw):
    tA, tB = LAYOUTS[layout]
    name = "%s-%s%s-%s-%dx%dx%d" % (group, what + "-" if what else "", "cfg%d" % cfg if cfg >= 0 else "auto", layout, M, N, K)
    return Case(group, name, cfg, tA, tB, M, N, K, **kw)


def cases_a(cfg, layout):
    """cfg x layout x loop edge: 1..7 k tiles with and without a partial last one, bias and D; one K without either and
    one K with D aliasing C"""
    BK = CFG[cfg][3]
    out = [_case("a", "", cfg, layout, M0, N0, K) for K in ks_for(BK)]
    out.append(_case("a", "plain", cfg, layout, M0, N0, 2 * BK + 4, bias=False, D="none"))
    out.append(_case("a", "alias", cfg, layout, M0, N0, 4 * BK - 4, D="alias"))
    return out


def cases_b(cfg, layout):
    """cfg x layout x split-K: a last slab 4 or 8 wide, an odd slab count, requests that collapse to fewer slabs and to
    one; bias and D present, so a slab other than 0 that adds them fails; the workspace is exactly split * M * N"""
    return [_case("b", "split%d" % s, cfg, layout, M0, N0, K, split=s) for K, s in SPLIT_PAIRS]


def cases_b_extra(layout):
    return [_case("b", "short-ws", 2, layout, M0, N0, 260, split=3, ws=-1, expect=ERR_WORKSPACE),
            _case("b", "short-ws-alias", -1, layout, M0, N0, 260, split=3, ws=-1, D="alias", expect=ERR_WORKSPACE),
            _case("b", "unsplit", 2, layout, M0, 202, 200, split=4),
            _case("b", "unsplit", -1, layout, M0, 202, 200, split=4)]


def cases_c(cfg):
    """the 16-dword epilogue behind the fast loaders: one thing at a time that switches vec_epi off, and a padded case
    that keeps it on"""
    out = []
    for layout in ("NN", "NT"):
        K = 2 * CFG[cfg][3] + 36
        out += [_case("c", "ldc+1", cfg, layout, M0, N0, K, pad=(0, 0, 1, 0)),
                _case("c", "C+1", cfg, layout, M0, N0, K, off=(0, 0, 1, 0, 0)),
                _case("c", "bias+1", cfg, layout, M0, N0, K, off=(0, 0, 0, 1, 0)),
                _case("c", "D+1-ldd+3", cfg, layout, M0, N0, K, pad=(0, 0, 0, 3), off=(0, 0, 0, 0, 1)),
                _case("c", "padded", cfg, layout, M0, N0, K, pad=(4, 8, 4, 12))]
    return out


EDGE_KS = (0, 1, 2, 3, 5, 33, 130)


def cases_d(layout):
    """the edge loader (launch_edge): whatever the configuration, forced or automatic"""
    tA, tB = LAYOUTS[layout]
    out = []
    for K in EDGE_KS:
        out.append(_case("d", "edge", -1, layout, M0, N0, K))
        out.append(_case("d", "edge", 16, layout, M0, N0, K))
    out += [_case("d", "edge-zeros", -1, layout, M0, N0, 0, bias=False, D="none"),
            _case("d", "edge-bias-only", -1, layout, M0, N0, 0, D="none"),
            _case("d", "edge-lda+1", -1, layout, M0, N0, 32, pad=(1, 0, 0, 0)),
            _case("d", "edge-lda+1", 12, layout, M0, N0, 96, pad=(1, 0, 0, 0)),
            _case("d", "edge-A+1", -1, layout, M0, N0, 32, off=(1, 0, 0, 0, 0)),
            _case("d", "edge-B+1", 23, layout, M0, N0, 32, off=(0, 1, 0, 0, 0)),
            _case("d", "edge-split-auto", -1, layout, 64, 64, 2050, split=0, auto=(3 if tA else 23, 8)),
            _case("d", "edge-split3", -1, layout, M0, N0, 262, split=3)]
    if layout == "TN":
        out.append(_case("d", "edge-M301", -1, layout, 301, N0, 32))
        out.append(_case("d", "edge-M301", 20, layout, 301, N0, 100))
    if layout == "NN":
        out.append(_case("d", "edge-N201", -1, layout, M0, 201, 32))
        out.append(_case("d", "edge-N201", 20, layout, M0, 201, 100))
    return out


def cases_empty():
    return [_case("d", "empty", -1, layout, M, N, 8, kinds=("exact",)) for layout in LAYOUTS for M, N in ((0, N0), (M0, 0))]


WALK_SHAPES = ((M0, N0), (520, 392))     # 520 x 392 on 64 x 64 tiles: 63 tiles, no multiple of 8


def cases_e(cfg, order):
    """the persistent walk (max_blocks) under both tile orders, with the 16-byte and the 16-dword epilogue (they have
    different barriers between tiles); the WGK > 1 classes ignore max_blocks and must still be right"""
    out = []
    K = 2 * CFG[cfg][3] + 36
    for M, N in WALK_SHAPES:
        for scalar in (False, True):
            base = _case("e", "", cfg, "NN", M, N, K, pad=(0, 0, 1 if scalar else 0, 0))
            for i, mb in enumerate((1, 3, 8, tiles(base) - 1)):
                layout = ("NN", "NT", "TN", "NN")[i]
                what = "order%d-mb%d%s" % (order, mb, "-scalar" if scalar else "")
                out.append(_case("e", what, cfg, layout, M, N, K, pad=(0, 0, 1 if scalar else 0, 0), max_blocks=mb, order=order))
    if cfg in WGK1_CLASS_CFGS:           # the walk crosses slabs
        base = _case("e", "", cfg, "NN", M0, N0, 260, split=3)
        for i, mb in enumerate((1, 3, 8, tiles(base) - 1)):
            layout = ("NT", "TN", "NN", "NT")[i]
            out.append(_case("e", "order%d-mb%d-split3" % (order, mb), cfg, layout, M0, N0, 260, split=3, max_blocks=mb, order=order))
    return out


def cases_e_knob():
    """vqa_gemm_set_max_blocks(n) + vqa_gemm_f32 against vqa_gemm_f32_ex(..., n): the same bits"""
    return [(_case("e", "knob-mb3", cfg, "NN", M0, N0, 100, max_blocks=3, entry="f32"),
             _case("e", "ex-mb3", cfg, "NN", M0, N0, 100, max_blocks=3)) for cfg in CLASS_CFGS]


def cases_f():
    """the automatic routes: one shape per branch of choose() and of the short-K hand-off that nothing else visits;
    exact data only.  auto = what choose() must answer (tests/test_gemm_reference.py holds the mirror above to it and
    the GPU test confirms the split through vqa_gemm_workspace_floats).

    NN 8192 x 1024 x 64 reaches configuration 22 only with the short-K hand-off switched off (K <= 304, N % 32 == 0: under
    the default mode gemm_shortk.hip takes it), so it runs under vqa_gemm_shortk_set_mode(0) like the configuration-13
    shape, and NN 8192 x 1024 x 308, the nearest K the hand-off refuses, reaches configuration 22 under the default
    mode: established by reading vqa_gemm_f32_ex (K <= 304 is the hand-off's own condition) and choose()."""
    f = lambda what, layout, M, N, K, **kw: _case("f", what, -1, layout, M, N, K, split=0, kinds=("exact",), **kw)
    out = [f("dx", "NT", 4096, 300, 2048, auto=(3, 4)),
           f("dWx", "TN", 300, 2048, 4096, auto=(21, 4)),
           f("cfg19", "TN", 2048, 2048, 4160, auto=(19, 2)),
           f("cfg22", "NN", 8192, 1024, 64, auto=(22, 1), shortk=0),
           f("cfg22-default-mode", "NN", 8192, 1024, 308, auto=(22, 1)),
           f("cfg13", "NN", 2304, 300, 64, auto=(13, 1), shortk=0)]
    for K in (4, 256, 260, 304, 308):
        out.append(f("shortk", "NN", 1024, 64, K, auto=(23, 1)))
        out.append(f("shortk-noD", "NN", 1024, 64, K, auto=(23, 1), D="none"))
    out.append(f("shortk-mb2", "NN", 1024, 64, 256, auto=(23, 1), max_blocks=2))
    return out


GATHER_SHAPES = ((3, 5, 200, 32, 4), (7, 36, 136, 96, 6), (9, 36, 264, 160, 20), (2, 1, 64, 64, 3))


def cases_g(tall):
    """vqa_gemm_f32_gather: M ragged against both BM, several n tiles (only the n0 == 0 tiles write gathered_out),
    1, 3, 5 and 2 k tiles"""
    out = []
    for B, R, N, K, ns in GATHER_SHAPES:
        for gout in ("none", "dense", "padded"):
            for bias in (False, True):
                pad = (4, 4, 4) if gout == "padded" else (0, 0, 0)
                name = "g-tall%d-%dx%dx%dx%d-%s%s" % (tall, B, R, N, K, gout, "-bias" if bias else "")
                out.append(GatherCase(name, tall, B, R, N, K, ns, gout, bias, pad))
    return out


def cases_g_refusals(tall):
    g = lambda what, N, K, code, **kw: GatherCase("g-tall%d-refuse-%s" % (tall, what), tall, 3, 5, N, K, 4, expect=code,
                                                  kinds=("exact",), **kw)
    return [g("K48", 200, 48, ERR_UNSUPPORTED, gout="dense"), g("N202", 202, 32, ERR_UNSUPPORTED, gout="dense"),
            g("lda+1", 200, 32, ERR_ALIGN, gout="dense", pad=(1, 0, 0)), g("gout+1", 200, 32, ERR_ALIGN, gout="offset")]


def matrix():
    """every Case and GatherCase of tests/test_gpu_gemm_f64.py"""
    out = []
    for cfg in range(NUM_CFG):
        for layout in LAYOUTS:
            out += cases_a(cfg, layout) + cases_b(cfg, layout)
    for layout in LAYOUTS:
        out += cases_b_extra(layout) + cases_d(layout)
    out += cases_empty()
    for cfg in CLASS_CFGS:
        out += cases_c(cfg)
        for order in (0, 1):
            out += cases_e(cfg, order)
    for knob, ex in cases_e_knob():
        out += [knob, ex]
    out += cases_f()
    for tall in (20, 21):
        out += cases_g(tall) + cases_g_refusals(tall)
    return out
