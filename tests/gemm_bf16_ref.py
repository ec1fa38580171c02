"""Float64 reference of the mixed-precision GEMM of include/vqa_hot.h (vqa_gemm_bf16, vqa_gemm_bf16_a16,
vqa_gemm_bf16_workspace_floats; csrc/gemm_bf16.hip), the data, the guarded buffers and the checks of its op-level test
(tests/test_gpu_gemm_bf16_f64.py), and the case matrix that crosses both entry points and the three layouts with every
edge of the kernel's loops.  Buffers, geometry and the exact comparator are those of tests/gemm_ref.py.

The contract:  ref64 = rne(op(A)) @ rne(op(B)) + bias + D  in float64, rne = bf16_ref.round_bf16 (nearest even), and the
yardstick of a rounding error  scale = |rne op(A)| @ |rne op(B)| + |bias| + |D|  (bf16_ref.gemm_scale without the two
epilogue terms makes a 1 x 1 x 1 product with bias and addend the worst case of tests/test_gpu_bf16.py; here the
epilogue's roundings are measured against what they round).

Three kinds of data for every case:
  exact   A, B, bias and D are independent integers in [-3, 3] (gemm_ref's).  Every one is a bf16 value and every partial
          sum of every order is an integer of magnitude <= 9 K + 6 < 2^24: every summation order, split and walk returns
          ref64 exactly.  Zero tolerance.
  ties    the same integers with every non-zero f32 entry of A and B moved onto a bf16 rounding tie that nearest-even
          sends back to the integer: half of them away from zero by 2^(e-8), e = floor(log2 |v|), the other half toward
          zero by the half-ulp of the binade they land in (2^(e-9) below a power of two, else 2^(e-8)):
              1 -> 1.00390625 | 0.998046875     2 -> 2.0078125 | 1.99609375     3 -> 3.0078125 | 2.9921875
          Truncation sends the toward-zero half to the integer's lower bf16 neighbour, round-half-away the other half to
          the upper one; either is then wrong by 2^-8 of an operand and more in most elements of C.  The reference is
          the `exact` reference and the comparator is equality.  A bf16 operand at rest (vqa_gemm_bf16_a16's A) holds the
          integers themselves; bias and D stay integers.
  real    standard normal operands (the a16 A rounded once on the host), judged element by element by the project's own
          bound  |got - ref64| <= bf16_ref.OP_TOL * scale.  Admission (tests/test_gemm_bf16_reference.py): the float32
          evaluation of the reference in both extreme orders of gemm_ref.ref32 lies within OP_TOL_MEASURED = OP_TOL / 3
          of ref64 -- the margin bf16_ref.py gives another legal summation order.  A case outside it would lose `real`
          (kinds) and keep the other two; none does.

Buffers: an operand whose leading dimension exceeds its width carries NaN (bf16: 0x7FC0) in the padding; C sits
NaN-filled between two NaN guards and its padding columns must still be NaN afterwards (an aliased addend occupies the
columns < N); a split-k workspace is NaN-filled, has exactly the floats the query reports and GUARD NaN floats behind
it: afterwards every float of it is a number (the reduction read nothing unwritten) and the guard is NaN.

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import dataclasses
import typing

import numpy as np
import torch

from tests import bf16_ref as B16
from tests import gemm_ref as G
from tests.gemm_ref import (GUARD, LAYOUTS, LAYOUT_OF, OK, ERR_WORKSPACE, c_buffer, geometry, pack, same_bits,  # noqa: F401
                            unpack_out, untouched)

OP_TOL = B16.OP_TOL
ADMIT = B16.OP_TOL_MEASURED      # what the float32 evaluations of a `real` case must stay inside
BM, BN, BK = 128, 128, 32        # the kernel's tile (csrc/gemm_bf16.hip); wave corner 64, MFMA 32, fetch quads of 4
KINDS = ("exact", "ties", "real")
ENTRIES = ("f32", "a16")
BF16_NAN = 0x7FC0


# -------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    """gemm_ref.Case's fields that apply, plus the entry point and a per-call max_blocks.  pad[0] and off[0] count
    elements of A as stored: floats for "f32" (off 0..1 past the 16-byte grid), bf16 for "a16" (off 0..3 past the 8-byte
    grid, lda odd or even and no multiple of 4)."""
    group: str
    name: str
    tA: int
    tB: int
    M: int
    N: int
    K: int
    split: int = 1               # the split_k argument (0: automatic)
    bias: bool = True
    D: str = "own"               # "own", "none", "alias" (D == C)
    pad: tuple = (0, 0, 0, 0)    # lda, ldb, ldc, ldd beyond the stored width
    off: tuple = (0, 0, 0, 0, 0)  # A, B, C, bias, D: elements past the aligned grid
    ws: typing.Optional[int] = 0  # workspace floats relative to what the plan needs (-1: one short); None: NULL
    max_blocks: int = 0
    entry: str = "f32"           # "f32": vqa_gemm_bf16, "a16": vqa_gemm_bf16_a16
    expect: int = OK
    kinds: tuple = KINDS

    def id(self):
        return self.name

    @property
    def layout(self):
        return LAYOUT_OF[(self.tA, self.tB)]


def cdiv(a, b):
    return -(-a // b)


def plan_split(M, N, K, split_k):
    """plan_split() of csrc/gemm_bf16.hip: (ranges, k per range)"""
    tiles = cdiv(M, BM) * cdiv(N, BN)
    s = split_k
    if s <= 0:
        s = min(512 // tiles, 8)
        s = min(s, K // 256)
    s = max(s, 1)
    per = max(cdiv(cdiv(K, s), BK) * BK, BK)
    return cdiv(K, per), per


def ranges(M, N, K, split_k):
    split, per = plan_split(M, N, K, split_k)
    return [(z * per, min(K, (z + 1) * per)) for z in range(split)]


def workspace_floats(M, N, K, split_k):
    split, _ = plan_split(M, N, K, split_k)
    return split * M * N if split > 1 else 0


def slabs(c):
    return plan_split(c.M, c.N, c.K, c.split)[0]


def units(c):
    """(range, tile) units of the launch"""
    return cdiv(c.M, BM) * cdiv(c.N, BN) * slabs(c)


# --------------------------------------------------------------------------------------------------------------- data
_DATA: dict = {}
_REF: dict = {}


def rne(x):
    """float32 array -> the nearest bf16 values (ties to even) as float32: bf16_ref.round_bf16"""
    return B16.round_bf16(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def truncated(x):
    return B16.truncate_bf16(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()


def half_away(x):
    """the other WRONG conversion: round to nearest, ties away from zero (half an ulp added to the magnitude, then cut)"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((bits + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32)


def to_ties(x, rng):
    """every non-zero integer of x moved onto the bf16 tie that nearest-even sends back to it (module docstring)"""
    a = np.abs(x).astype(np.float64)
    nz = a > 0
    e = np.floor(np.log2(np.where(nz, a, 1.0)))
    away = rng.random_sample(x.shape) < 0.5
    below = np.where(a == 2.0 ** e, 2.0 ** (e - 9), 2.0 ** (e - 8))
    moved = np.where(away, a + 2.0 ** (e - 8), a - below)
    out = np.where(nz, np.sign(x) * moved, 0.0).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.where(nz, np.sign(x) * moved, 0.0))      # float32 holds them
    return out


def operands(c, kind):
    """the logical operands {A [M,K], B [K,N], bias [N], D [M,N]} (float32) the entry point is handed: for "a16" A holds
    bf16 values.  Cases of one shape, layout and entry share them."""
    key = (kind, c.entry == "a16", c.tA, c.tB, c.M, c.N, c.K)
    if key not in _DATA:
        d = dict(G.operands(c, "real" if kind == "real" else "exact"))
        if kind == "ties":
            rng = G._rng("ties", c.tA, c.tB, c.M, c.N, c.K)
            a, b = to_ties(d["A"], rng), to_ties(d["B"], rng)
            d["A"], d["B"] = (d["A"] if c.entry == "a16" else a), b
        elif kind == "real" and c.entry == "a16":
            d["A"] = rne(d["A"])
        _DATA[key] = d
    return _DATA[key]


def contract(d, bias=True, D=True):
    """(ref64, scale) of operands: the header's contract evaluated as it is written"""
    a, b = rne(d["A"]), rne(d["B"])
    bv, dv = (d["bias"] if bias else None), (d["D"] if D else None)
    return (G._product(a, b, bv, dv),
            G._product(np.abs(a), np.abs(b), None if bv is None else np.abs(bv), None if dv is None else np.abs(dv)))


def ref(c, kind):
    """(ref64 [M,N], scale [M,N]).  `ties` is judged against the `exact` reference (the comparator ignores its scale);
    the rounding is idempotent, so both entries share the `real` reference of a shape."""
    if kind != "real":
        return G.ref(c, "exact")
    key = (c.tA, c.tB, c.M, c.N, c.K, c.bias, c.D != "none")
    if key not in _REF:
        _REF[key] = contract(G.operands(c, "real"), c.bias, c.D != "none")
    return _REF[key]


def bits16(x):
    """float32 array of bf16 values -> their 16-bit patterns"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not bf16 values"
    return (u >> 16).astype(np.uint16)


def pack16(arr, ld, off=0):
    """gemm_ref.pack for a bf16 operand at rest: 16-bit patterns, NaN (0x7FC0) in the padding; the buffer's own start is
    taken to be 16-byte aligned, so `off` elements is the misalignment against the 8-byte grid"""
    arr = np.atleast_2d(arr)
    rows, width = arr.shape
    buf = np.full(max(off + rows * ld, 8), BF16_NAN, np.uint16)
    buf[off:off + rows * ld].reshape(rows, ld)[:, :width] = bits16(arr)
    return buf


def pack_a(c, ops):
    """A as the entry point reads it: (flat buffer, bytes per element)"""
    _, _, lda, off = geometry(c)["A"]
    stored = ops["A"].T if c.tA else ops["A"]
    return (pack16(stored, lda, off), 2) if c.entry == "a16" else (pack(stored, lda, off), 4)


def ws_buffer(need):
    """the NaN-filled workspace of `need` floats with its guard behind"""
    return np.full(need + GUARD, np.nan, np.float32)


# ------------------------------------------------------------------------------------------------------------- checks
def compare(got, r64, scale, kind, what):
    """exact, ties: got == ref64 element for element (gemm_ref's comparator); real: |got - ref64| <= OP_TOL * scale.
    Returns the worst error as a fraction of the bound (0 for exact data).  A NaN fails both."""
    if kind != "real":
        return G.compare(got, r64, scale, "exact", 0, 1, what)
    if got.shape != r64.shape:
        raise AssertionError("%s: shape %s, want %s" % (what, got.shape, r64.shape))
    bound = OP_TOL * scale
    err = np.abs(got.astype(np.float64) - r64)
    bad = ~(err <= bound)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("%s: outside %.3g * scale: %s (got %r, want %r, error %.3g, bound %.3g)"
                             % (what, OP_TOL, G._where(bad), got[i, j], r64[i, j], err[i, j], bound[i, j]))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def check_workspace(ws_after, need, what, written=True):
    """ws_after: the need + GUARD floats of ws_buffer() after the call"""
    assert ws_after.shape == (need + GUARD,)
    if not np.isnan(ws_after[need:]).all():
        raise AssertionError("%s: wrote behind the workspace (its guard is no longer NaN)" % what)
    nan = np.isnan(ws_after[:need])
    if written and nan.any():
        raise AssertionError("%s: %d workspace floats were never written, first at %d" % (what, nan.sum(), np.argmax(nan)))
    if not written and not nan.all():
        raise AssertionError("%s: the workspace was written by a refused call" % what)


def check_run(c, kind, ops, c_after, start, ws_after, what):
    """one finished call, from host copies of its guarded C buffer and (split k) its workspace: guards, padding columns,
    workspace and the result against the reference.  Returns (C [M,N], worst error as a fraction of the bound)."""
    ldc = geometry(c)["C"][2]
    if c.expect != OK:
        untouched(c, c_after, start, ops, what)
        if ws_after is not None:
            check_workspace(ws_after, len(ws_after) - GUARD, what, written=False)
        return None, 0.0
    got = unpack_out(c_after, start, c.M, c.N, ldc, what).copy()
    need = workspace_floats(c.M, c.N, c.K, c.split)
    if need:
        check_workspace(ws_after, need, what)
    r64, scale = ref(c, kind)
    return got, compare(got, r64, scale, kind, what)


def real_condition(cases):
    """the admission of the `real` cases: (worst |ref32 - ref64| / scale over both orders, where) over the distinct
    problems, and the ids of the cases outside ADMIT"""
    worst, at, seen, outside = 0.0, None, {}, []
    for c in cases:
        if "real" not in c.kinds or c.expect != OK:
            continue
        key = (c.tA, c.tB, c.M, c.N, c.K, c.bias, c.D != "none")
        if key not in seen:
            d = G.operands(c, "real")
            rounded = {"A": rne(d["A"]), "B": rne(d["B"]), "bias": d["bias"], "D": d["D"]}
            r64, scale = ref(c, "real")
            assert (scale > 0).all()
            x, xo = 0.0, None
            for order in ("seq", "chunk8"):
                e = float((np.abs(G.ref32(c, "real", order, rounded).astype(np.float64) - r64) / scale).max())
                if e > x:
                    x, xo = e, order
            seen[key] = (x, xo)
        x, xo = seen[key]
        if x > ADMIT:
            outside.append(c.id())
        if x > worst:
            worst, at = x, "%s (%s)" % (c.id(), xo)
    return worst, at, outside


# -------------------------------------------------------------------------------------------------------- case matrix
def _case(group, what, entry, layout, M, N, K, **kw):
    tA, tB = LAYOUTS[layout]
    name = "%s-%s%s-%s-%dx%dx%d" % (group, what + "-" if what else "", entry, layout, M, N, K)
    return Case(group, name, tA, tB, M, N, K, entry=entry, **kw)


KS_A = (1, 2, 3, 4, 5, 31, 32, 33, 36, 63, 64, 65, 95, 96, 97, 128, 130)
EDGES_B = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
SHAPES_C = ((67, 70, 77), (68, 72, 80))
SHAPE_D = (130, 70, 100)
KS_E = (33, 64, 65, 300, 544)
REQUESTS_E = (2, 3, 4, 8, 64)
AUTO_F = (((128, 128, 511), 1, 512), ((128, 128, 512), 2, 256), ((40, 36, 2100), 8, 288))      # shape, ranges, k per range
WALKS_G = (((257, 130, 100), 1, 6), ((257, 130, 200), 3, 18))                                   # shape, request, units


def cases_a(entry, layout):
    """the k loop in one range: 1..5 k tiles with and without a partial last tile and a partial quad; nk == 1 (no
    prefetch), nk == 2 (the second tile waits in registers), the steady state"""
    return [_case("a", "", entry, layout, 33, 65, K) for K in KS_A]


def cases_b(entry, layout):
    """M and N on the quad, MFMA, wave-corner and tile boundaries and beside them; two k tiles, the last partial"""
    return ([_case("b", "M", entry, layout, M, 36, 40) for M in EDGES_B] +
            [_case("b", "N", entry, layout, 36, N, 40) for N in EDGES_B])


def loader_combos(entry):
    """(padA, offA, padB, offB): each operand on its own through every base and leading dimension, the other dense and
    aligned; the first one is the all-aligned dense call"""
    a = [(p, o) for p in ((0, 4, 1, 2) if entry == "a16" else (0, 4, 1)) for o in (range(4) if entry == "a16" else range(2))]
    b = [(p, o) for p in (0, 4, 1) for o in range(2)]
    return [(p, o, 0, 0) for p, o in a] + [(0, 0, p, o) for p, o in b[1:]]


def cases_c(entry, layout, shape):
    M, N, K = shape
    return [_case("c", "lda+%d-A+%d-ldb+%d-B+%d" % (pa, oa, pb, ob), entry, layout, M, N, K, pad=(pa, pb, 0, 0),
                  off=(oa, ob, 0, 0, 0)) for pa, oa, pb, ob in loader_combos(entry)]


def cases_d(entry, layout):
    """the epilogue: bias x addend (none, its own buffer with ldd != ldc, C itself) x ldc x C's alignment"""
    M, N, K = SHAPE_D
    out = []
    for bias in (True, False):
        for D in ("none", "own", "alias"):
            for padc in (0, 5):
                for offc in (0, 1):
                    what = "%s-D%s-ldc+%d-C+%d" % ("bias" if bias else "nobias", D, padc, offc)
                    out.append(_case("d", what, entry, layout, M, N, K, bias=bias, D=D, pad=(0, 0, padc, padc + 3),
                                     off=(0, 0, offc, 0, 0)))
    return out


def cases_e(entry, layout):
    """requested split k: requests above the number of k tiles, a last range of one partial tile, bias in slab 0, the
    addend (its own, and C itself under ldc > N) in the reduction"""
    M, N = SHAPE_D[:2]
    out = []
    for K in KS_E:
        for s in REQUESTS_E:
            out.append(_case("e", "split%d" % s, entry, layout, M, N, K, split=s))
            out.append(_case("e", "split%d-alias-ldc+5" % s, entry, layout, M, N, K, split=s, D="alias", pad=(0, 0, 5, 0)))
    return out


def cases_e_refusals(entry, layout):
    M, N = SHAPE_D[:2]
    r = lambda what, **kw: _case("e", what, entry, layout, M, N, 300, split=3, expect=ERR_WORKSPACE, kinds=("exact",), **kw)
    return [r("short-ws", ws=-1), r("short-ws-alias", ws=-1, D="alias", pad=(0, 0, 5, 0)), r("null-ws", ws=None),
            r("null-ws-alias", ws=None, D="alias")]


def cases_f(entry, layout):
    return [_case("f", "auto", entry, layout, M, N, K, split=0) for (M, N, K), _, _ in AUTO_F]


def cases_g(entry, layout):
    """the persistent walk within one range and across slabs (bias in slab 0, the addend its own and C itself):
    [(the max_blocks = 0 twin, [walks])]"""
    out = []
    for (M, N, K), req, n in WALKS_G:
        for D in (("own",) if req == 1 else ("own", "alias")):
            mk = lambda mb: _case("g", "split%d-D%s-mb%d" % (req, D, mb), entry, layout, M, N, K, split=req, D=D, max_blocks=mb)
            out.append((mk(0), [mk(mb) for mb in (1, 3, n - 1, n, n + 7)]))
    return out


FAMILIES = "abcdefg"


def family(group, entry, layout):
    """the flat cases of one family for one entry and layout"""
    if group == "c":
        return [c for shape in SHAPES_C for c in cases_c(entry, layout, shape)]
    if group == "e":
        return cases_e(entry, layout) + cases_e_refusals(entry, layout)
    if group == "g":
        return [c for twin, walks in cases_g(entry, layout) for c in [twin] + walks]
    return {"a": cases_a, "b": cases_b, "d": cases_d, "f": cases_f}[group](entry, layout)


def matrix():
    """every Case of tests/test_gpu_gemm_bf16_f64.py"""
    return [c for group in FAMILIES for entry in ENTRIES for layout in LAYOUTS for c in family(group, entry, layout)]
