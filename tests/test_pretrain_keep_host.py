"""Host side of the pre-training steps' seeded dropout (no GPU): the stream layout PretrainEngine.keep_offsets against an
independent restatement of the three counter regions, struct vqa_pretrain_keep_t against the header, and the argument
checks of the vqa_pretrain_*_ex entry points, which run before any HIP call."""
import ctypes as C
import os
import re
import types

import pytest

from vqa_transfer_externaldata_amd import pretrain as PT

KINDS = ("obj", "attr")
DIMS = dict(n=5, R=36, H=1024)
SMALL = dict(n=5, R=6, H=8)
# (heads, noc): cfg-5 (and adapt, the same head set), the two enwiki models, the two noc models
MODELS = [(("bf", "ws"), False), (("bf", "ws", "ew"), False), (("bf", "ew"), False), (("bf", "ws"), True), (("bf", "ew"), True)]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from vqa_transfer_externaldata_amd import _lib
    return _lib


def _offsets(dims, heads, noc, B, step, row_offset=0, global_rows=None):
    """PretrainEngine.keep_offsets needs the engine's dims and head set only: called on a stand-in, so without a GPU"""
    stub = types.SimpleNamespace(heads=tuple(heads), noc=noc, **dims)
    return PT.PretrainEngine.keep_offsets(stub, B, step, row_offset, global_rows)


def _restated(n, R, H, heads, noc, B, step, row_offset, Bg):
    """The three counter regions written out, site by site (the layout make_keep_masks has drawn since the models exist).
    Region 1, from 0: per step one block of 2 categories x (att + bf_joint + ws_joint), every site Bg images long.
    Region 2, from 2^62: per step 2 categories x ew_joint.  Region 3, from 2^61: per step, head by head, 2 categories x the
    l branch's joint.  A shard starts row_offset images into each site."""
    att, joint = n * R * H, n * 2 * H
    out = {}
    per_kind = Bg * att + Bg * joint + Bg * joint
    base = step * 2 * per_kind
    for ki, k in enumerate(KINDS):
        b = base + ki * per_kind
        out[k + "/att"] = (b + row_offset * att, att, 0.8)
        out[k + "/bf_joint"] = (b + Bg * att + row_offset * joint, joint, 0.5)
        out[k + "/ws_joint"] = (b + Bg * att + Bg * joint + row_offset * joint, joint, 0.5)
    if "ew" in heads:
        base = 2 ** 62 + step * 2 * Bg * joint
        for ki, k in enumerate(KINDS):
            out[k + "/ew_joint"] = (base + ki * Bg * joint + row_offset * joint, joint, 0.5)
    if noc:
        base = 2 ** 61 + step * 2 * len(heads) * Bg * joint
        for hi, h in enumerate(heads):
            for ki, k in enumerate(KINDS):
                out["%s/%s_joint_l" % (k, h)] = (base + (2 * hi + ki) * Bg * joint + row_offset * joint, joint, 0.5)
    return out


@pytest.mark.parametrize("dims", [DIMS, SMALL], ids=["H1024", "H8"])
@pytest.mark.parametrize("heads,noc", MODELS, ids=["-".join(h) + ("-noc" if c else "") for h, c in MODELS])
def test_keep_offsets_equal_the_restated_regions(heads, noc, dims):
    for step in (0, 1, 7):
        for B, row_offset, global_rows in ((16, 0, None), (8, 8, 16), (3, 2, 5), (512, 0, 512)):
            got = _offsets(dims, heads, noc, B, step, row_offset, global_rows)
            want = _restated(heads=heads, noc=noc, B=B, step=step, row_offset=row_offset,
                             Bg=B if global_rows is None else global_rows, **dims)
            assert got == want, (step, B, row_offset, global_rows)
            assert all(off % 4 == 0 for off, _, _ in got.values())      # H % 4 == 0: every site starts on a mask word
            # the sites of one step, and of the next step, do not overlap: [offset, offset + B * per image) are disjoint
            spans = sorted((off, off + B * per) for off, per, _ in
                           list(got.values()) + list(_offsets(dims, heads, noc, B, step + 1, row_offset, global_rows).values()))
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (step, B)
    # a shard's site starts where the whole batch's rows of that shard start
    whole = _offsets(dims, heads, noc, 16, 3)
    shard = _offsets(dims, heads, noc, 8, 3, row_offset=8, global_rows=16)
    assert all(shard[k][0] == whole[k][0] + 8 * whole[k][1] for k in whole)


def test_site_names_are_those_of_make_keep_masks():
    assert sorted(_offsets(SMALL, ("bf", "ws"), False, 3, 0)) == sorted(k + s for k in KINDS for s in ("/att", "/bf_joint", "/ws_joint"))
    ew = _offsets(SMALL, ("bf", "ew"), False, 3, 0)
    assert "obj/ew_joint" in ew and "attr/ws_joint" in ew          # the cfg-5 region keeps its layout without the ws head
    noc = _offsets(SMALL, ("bf", "ew"), True, 3, 0)
    assert {"obj/bf_joint_l", "attr/ew_joint_l"} <= set(noc) and "obj/ws_joint_l" not in noc


def test_struct_sizes_and_the_keep_struct_match_the_header(built, repo_root):
    L = built
    # the existing batch structs did not grow (the mask pointers live in nested structs that cannot grow at their ends)
    P = C.sizeof(C.c_void_p)
    assert C.sizeof(L.PtKind) == 9 * P and C.sizeof(L.PtBatch) == (3 + 2 * 9 + 3) * P
    assert C.sizeof(L.PtCtxKind) == 3 * P and C.sizeof(L.PtExtBatch) == C.sizeof(L.PtBatch) + (2 * 3 + 3) * P
    assert C.sizeof(L.PtNocKind) == 3 * P and C.sizeof(L.PtNocBatch) == C.sizeof(L.PtExtBatch) + 2 * 3 * P
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "vqa_hot.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} vqa_pretrain_keep_t;", src).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, rest = decl.split(None, 1)
        m = re.match(r"(\w+)((?:\[\d+\])*)$", rest.strip())
        fields.append((m.group(1), typ, [int(x) for x in re.findall(r"\[(\d+)\]", m.group(2))]))
    ctype = {"uint64_t": C.c_uint64, "int32_t": C.c_int32}
    assert [f[0] for f in fields] == [f[0] for f in L.PtKeep._fields_]
    for (name, typ, dims), (pname, ptype) in zip(fields, L.PtKeep._fields_):
        want = ctype[typ]
        for d in reversed(dims):
            want = want * d
        assert pname == name and C.sizeof(ptype) == C.sizeof(want), name
        elem = ptype
        for _ in dims:
            elem = elem._type_
        assert elem is ctype[typ], name
    assert C.sizeof(L.PtKeep) == 8 * (1 + 4 * 2 + 6) + 8            # the int32 and its padding
    bits = dict(re.findall(r"#define VQA_PT_KEEP_SITE_(\w+) (\d+)", src))
    assert {k.lower(): int(v) for k, v in bits.items() if k != "ALL"} == L.PT_KEEP_SITE
    assert int(bits["ALL"]) == sum(L.PT_KEEP_SITE.values())


def _ext_dims(L, heads):
    base = L.PtDims(B=2, n=5, R=6, D=16, H=8, W=12, A=12, Vq=20, n_ws=7, L=4, flags=0, keep_att=0.8, keep_joint=0.5)
    return L.PtExtDims(base=base, heads=heads, Lc=7, n_ctx=15)


# family -> (dims, params struct, batch struct, where the ext batch sits in it)
def _family(L, fam):
    if fam == "vqa_pretrain_":
        return _ext_dims(L, 3).base, L.PtParams(), L.PtBatch(), lambda b: b.kind
    if fam == "vqa_pretrain_ext_":
        return _ext_dims(L, 7), L.PtExtParams(), L.PtExtBatch(), lambda b: b.base.kind
    if fam == "vqa_pretrain_noc_":
        return _ext_dims(L, 3), L.PtNocParams(), L.PtNocBatch(), lambda b: b.base.base.kind
    P = L.PtAdaptParams()       # the adapt entry points check the v_adapt members with their first arguments
    P.v_adapt.w = P.v_adapt.b = 64
    for i in range(2):
        P.v_adapt.gamma[i] = P.v_adapt.beta[i] = 64
    return _ext_dims(L, 3), P, L.PtExtBatch(), lambda b: b.base.kind


@pytest.mark.parametrize("fam", ["vqa_pretrain_", "vqa_pretrain_ext_", "vqa_pretrain_noc_", "vqa_pretrain_adapt_"])
def test_ex_entry_points_check_their_arguments_before_any_hip_call(built, fam):
    """Workspace pointer 16 with 0 bytes: a call whose other arguments pass is refused for the workspace (-5) before any
    launch, so the codes here come from the host-only checks alone (as tests/test_abi.py does for the ops)"""
    L = built
    lib = L.load()
    d, P, b, kinds = _family(L, fam)
    fwd, fwd_ex = getattr(lib, fam + "forward"), getattr(lib, fam + "forward_ex")
    bwd, bwd_ex = getattr(lib, fam + "backward_phases"), getattr(lib, fam + "backward_phases_ex")
    ws = C.c_void_p(16)
    zero = L.PtKeep()
    plain = fwd(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None)
    assert plain == -5
    assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, None) == plain
    assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(zero)) == plain
    plain = bwd(C.byref(d), C.byref(P), C.byref(P), C.byref(b), ws, 0, None, 15, None)
    assert plain == -5
    assert bwd_ex(C.byref(d), C.byref(P), C.byref(P), C.byref(b), ws, 0, None, 15, None, None) == plain
    assert bwd_ex(C.byref(d), C.byref(P), C.byref(P), C.byref(b), ws, 0, None, 15, None, C.byref(zero)) == plain
    # NULL dims / batch: VQA_ERR_ARG from both forms
    assert fwd(None, C.byref(P), C.byref(b), ws, 0, 1, None) == fwd_ex(None, C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(zero)) == -1
    # every site seeded, no mask pointer: passes the keep check (the workspace is refused next) ...
    seeded = L.PtKeep(keep_seed=9, seeded=sum(L.PT_KEEP_SITE.values()))
    assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(seeded)) == -5
    # ... a seeded site that also has a mask pointer is VQA_ERR_ARG, in the forward and the backward
    for member, bit in (("keep_att", 1), ("keep_bf_joint", 2), ("keep_ws_joint", 4)):
        setattr(kinds(b)[1], member, 64)
        one = L.PtKeep(keep_seed=9, seeded=bit)
        assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(one)) == -1, member
        assert bwd_ex(C.byref(d), C.byref(P), C.byref(P), C.byref(b), ws, 0, None, 15, None, C.byref(one)) == -1, member
        other = L.PtKeep(keep_seed=9, seeded=sum(L.PT_KEEP_SITE.values()) & ~bit)       # the mask's own site explicit: fine
        assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(other)) == -5, member
        setattr(kinds(b)[1], member, None)
    if fam != "vqa_pretrain_":
        ext = b.base if fam == "vqa_pretrain_noc_" else b
        ext.ctx[0].keep_ew_joint = 64
        assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(L.PtKeep(seeded=8))) == -1
        ext.ctx[0].keep_ew_joint = None
    if fam == "vqa_pretrain_noc_":
        b.l[1].keep_ws_l_joint = 64
        assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(L.PtKeep(seeded=16))) == -1
        b.l[1].keep_ws_l_joint = None
    # an unknown site bit
    assert fwd_ex(C.byref(d), C.byref(P), C.byref(b), ws, 0, 1, None, C.byref(L.PtKeep(seeded=32))) == -1


def test_trainer_flag_and_engine_signatures():
    import inspect
    from vqa_transfer_externaldata_amd import pretrain_trainer as T
    assert T.build_parser().parse_args(["--inline_dropout"]).inline_dropout and not T.build_parser().parse_args([]).inline_dropout
    for fn in (PT.PretrainEngine.forward, PT.PretrainEngine.train_step):
        sig = inspect.signature(fn)
        assert sig.parameters["dropout"].default is None and "row_offset" in sig.parameters and "global_rows" in sig.parameters
