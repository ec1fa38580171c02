"""Seeded dropout of the pre-training steps: the keep bits computed inside the kernels that serve several queries per
memory (vqa_attn_pool_fwd_rep_seeded / vqa_attn_pool_bwd_rep_seeded, rep 1..8) and inside every dropout site of the four step
families (vqa_pretrain_forward_ex, vqa_pretrain_backward_phases_ex, vqa_pretrain_ext_forward_ex,
vqa_pretrain_ext_backward_phases_ex, vqa_pretrain_noc_forward_ex, vqa_pretrain_noc_backward_phases_ex,
vqa_pretrain_adapt_forward_ex, vqa_pretrain_adapt_backward_phases_ex; struct vqa_pretrain_keep_t;
PretrainEngine.train_step(dropout=(seed, step)); config.inline_dropout).

The reference everywhere is the explicit-mask twin on the mask ops.dropout_mask(n, seed, offset, keep, device) writes: the
same kernel reads from a buffer the word the seeded form computes.  Every comparison is torch.equal; there is no tolerance."""
import numpy as np
import pytest
import torch

from oracle import pretrain_oracle as PO
from tests import pretrain_adapt_ref as AR
from tests import pretrain_enwiki_ref as ER
from tests import pretrain_noc_ref as NR

pytestmark = pytest.mark.gpu

SEED = 123
OFFSETS = (0, 4 * 12345, (3 << 40) + 28)
KEEPS = (0.8, 0.5, 1.0)


def _ops():
    from vqa_transfer_externaldata_amd import ops
    return ops


def _lib():
    from vqa_transfer_externaldata_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def _same(x, y, what):
    assert len(x) == len(y)
    for i, (a, b) in enumerate(zip(x, y)):
        assert torch.equal(a, b), what + (i,)


# ------------------------------------------------------------------------------------------------------ the ops
# (name, B, rep, R, H, D, vqa_attn_set_fast or None).  Forward route / backward route of each:
#   rep-fwd-*     the per-memory forward attn_pool_fwd_form_kernel<FwdRep, H / 256, D, .>; R 3: fewer rows than its prefetch
#                 depth of 4, R 9 and R 40: the edges of the 8-row wave stride and the 6-row pooling batch.  Backward: generic
#                 attn_pool_bwd_kernel<5> (H 256; D 4096)
#   d1024         attn_pool_fwd_form_kernel<FwdRepD1024, 4, 1024, .> / attn_pool_bwd_fast_kernel<5, ., 1024>
#   fast-bwd      attn_pool_bwd_fast_kernel<5, ., 2048> (forward: attn_pool_fwd_form_kernel<FwdRep, 4, 2048, .>)
#   generic       attn_pool_fwd_kernel with rep / attn_pool_bwd_kernel<5> (rep 2, 5) and <8> (rep 8)
#   generic-big   the generic pair at a models' shape under vqa_attn_set_fast(0)
#   per-query     attn_pool_fwd_form_kernel<FwdFast, ...> with rep > 1 under vqa_attn_set_fast(2) (rep 3) and (3) (rep 5)
ATT_CASES = [("rep-fwd-h256-d2048-R%d" % R, 3, 5, R, 256, 2048, None) for R in (36, 3, 9, 40)] + \
            [("rep-fwd-h1024-d4096-R%d" % R, 2, 5, R, 1024, 4096, None) for R in (36, 3, 9, 40)] + \
            [("d1024", 2, 5, 36, 1024, 1024, None), ("fast-bwd-R36", 2, 5, 36, 1024, 2048, None),
             ("fast-bwd-R5", 2, 5, 5, 1024, 2048, None)] + \
            [("generic-rep%d" % rep, 3, rep, 6, 8, 16, None) for rep in (2, 5, 8)] + \
            [("generic-big", 2, 5, 36, 256, 2048, 0), ("per-query-fast2-rep3", 2, 3, 36, 256, 2048, 2),
             ("per-query-fast3-rep5", 2, 5, 36, 256, 2048, 3)]


def _att_case(B, rep, Rg, H, D, seed=7):
    g = torch.Generator().manual_seed(seed)
    v, qv, w, bias = _randn(g, B, Rg, H), _randn(g, B * rep, H), _randn(g, H), _randn(g, 1)
    V, dpooled = _randn(g, B, Rg, D), _randn(g, B * rep, D)
    nb = torch.tensor(([Rg, 1, Rg // 2 + 1, Rg] * B)[:B], dtype=torch.int32).cuda()      # full and short counts, one of 1
    return v, qv, V, nb, w, bias, dpooled


@pytest.mark.parametrize("name,B,rep,Rg,H,D,fast", ATT_CASES, ids=[c[0] for c in ATT_CASES])
def test_attention_rep_seeded_equals_explicit(name, B, rep, Rg, H, D, fast):
    ops, lib = _ops(), _lib().load()
    v, qv, V, nb, w, bias, dpooled = _att_case(B, rep, Rg, H, D)
    if fast is not None:
        lib.vqa_attn_set_fast(fast)
    try:
        for off in OFFSETS:
            for keep in KEEPS:
                mask = ops.dropout_mask(B * rep * Rg * H, SEED, off, keep, "cuda")
                x = ops.attn_pool_fwd_rep(v, qv, V, nb, w, bias, rep, keepmask=mask, keep_prob=keep)
                y = ops.attn_pool_fwd_rep(v, qv, V, nb, w, bias, rep, keep_seed=(SEED, off), keep_prob=keep)
                _same(x, y, (name, "fwd att, pooled", off, keep))
                assert torch.isfinite(x[1]).all()
                x = ops.attn_pool_bwd_rep(dpooled, v, qv, V, x[0], w, rep, keepmask=mask, keep_prob=keep, parts=True)
                y = ops.attn_pool_bwd_rep(dpooled, v, qv, V, y[0], w, rep, keep_seed=(SEED, off), keep_prob=keep, parts=True)
                _same(x, y, (name, "bwd dv, dqv, part_dw, part_db", off, keep))
                assert all(torch.isfinite(t).all() for t in x)
        # the mask matters, and every query has its own: another seed gives other scores for each of the rep queries
        a = ops.attn_pool_fwd_rep(v, qv, V, nb, w, bias, rep, keep_seed=(SEED, 0), keep_prob=0.5)[0].view(B, rep, Rg)
        b = ops.attn_pool_fwd_rep(v, qv, V, nb, w, bias, rep, keep_seed=(SEED + 1, 0), keep_prob=0.5)[0].view(B, rep, Rg)
        if Rg > 1:
            assert all(not torch.equal(a[0, j], b[0, j]) for j in range(rep))
    finally:
        lib.vqa_attn_set_fast(1)


def test_refusals_of_the_seeded_rep_calls():
    ops, L = _ops(), _lib()
    lib = L.load()
    B, rep, Rg, H, D = 2, 5, 4, 8, 12
    v, qv, V, nb, w, bias, dpooled = _att_case(B, rep, Rg, H, D)
    att, pooled = torch.empty(B * rep, Rg).cuda(), torch.empty(B * rep, D).cuda()
    p = lambda t: t.data_ptr()
    V16 = V.to(torch.bfloat16)
    # several queries per memory read an f32 memory only: the entry points with a bf16 memory refuse rep 5
    with pytest.raises(L.VqaHotError, match="unsupported"):
        L.check(lib.vqa_attn_pool_fwd_seeded(p(v), p(qv), p(V16), 1, p(nb), p(w), p(bias), SEED, 0, 0.8, p(att), p(pooled), B,
                                             rep, Rg, H, D, None), "vqa_attn_pool_fwd_seeded")
    dv, dqv, pdw, pdb = torch.empty_like(v), torch.empty_like(qv), torch.empty(B * rep, H).cuda(), torch.empty(B * rep).cuda()
    with pytest.raises(L.VqaHotError, match="unsupported"):
        L.check(lib.vqa_attn_pool_bwd_seeded(p(dpooled), p(v), p(qv), p(V16), 1, p(att), p(w), SEED, 0, 0.8, p(dv), p(dqv),
                                             p(pdw), p(pdb), B, rep, Rg, H, D, None), "vqa_attn_pool_bwd_seeded")
    with pytest.raises(L.VqaHotError, match="aligned"):
        ops.attn_pool_fwd_rep(v, qv, V, nb, w, bias, rep, keep_seed=(SEED, 2), keep_prob=0.8)
    with pytest.raises(L.VqaHotError, match="aligned"):
        ops.attn_pool_bwd_rep(dpooled, v, qv, V, att, w, rep, keep_seed=(SEED, 2), keep_prob=0.8)
    mask = ops.dropout_mask(B * rep * Rg * H, SEED, 0, 0.8, "cuda")
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.attn_pool_fwd_rep(v, qv, V, nb, w, bias, rep, keepmask=mask, keep_seed=(SEED, 0), keep_prob=0.8)


# ------------------------------------------------------------------------------------------------------ the engines
TOY = dict(B=3, n=5, R=6, D=16, H=8, L=4, W=12, Vq=20, n_ws=7, A=12)
MID = dict(B=16, n=5, R=36, D=256, H=128, L=10, W=300, Vq=200, n_ws=50, A=400)
# H 1024, R 36: the per-memory rep kernels inside a step -- D 2048 (cfg-5: attn_pool_fwd_form_kernel<FwdRep, 4, 2048, .> and
# attn_pool_bwd_fast_kernel<5, ., 2048>) and the 1024-wide adapted memory (the d1024 pair)
WIDE = dict(B=2, n=5, R=36, D=2048, H=1024, L=4, W=12, Vq=20, n_ws=7, A=12)
WIDE_ADAPT = dict(WIDE, D=64)
CTX = {"n_ctx": 15, "Lc": 7}
# model -> (head set, noc, adapt, the entry points its engine calls)
MODELS = {"cfg5": (("bf", "ws"), False, False, "vqa_pretrain_"),
          "bf_ws_ew": (("bf", "ws", "ew"), False, False, "vqa_pretrain_ext_"),
          "bf_ew": (("bf", "ew"), False, False, "vqa_pretrain_ext_"),
          "noc_bf_ws": (("bf", "ws"), True, False, "vqa_pretrain_noc_"),
          "noc_bf_ew": (("bf", "ew"), True, False, "vqa_pretrain_noc_"),
          "adapt": (("bf", "ws"), False, True, "vqa_pretrain_adapt_")}


def _model_case(model, cfg, ln_shared=True, seed=11, precision="f32"):
    """(parameters, host batch, engine factory) of one of the six native pre-training models"""
    from vqa_transfer_externaldata_amd import pretrain as PT
    heads, noc, adapt, _ = MODELS[model]
    c = dict(cfg)
    B, n, R, D, H, L, W, Vq, n_ws, A = (c[k] for k in ("B", "n", "R", "D", "H", "L", "W", "Vq", "n_ws", "A"))
    rng = np.random.default_rng(seed)
    nc = CTX["n_ctx"] if "ew" in heads else None
    kw = dict(W=W, D=D, H=H, ln_shared=ln_shared)
    if noc:
        p = NR.init_params(rng, Vq, n_ws, A, heads=heads, n_ctx=nc, **kw)
    elif adapt:
        p = AR.init_params(rng, Vq, n_ws, A, **kw)
    elif heads == ("bf", "ws"):
        p = PO.init_params(rng, Vq, n_ws, A, **kw)
    else:
        p = ER.init_params(rng, Vq, n_ws, A, heads=heads, n_ctx=nc, **kw)
    batch = PO.make_batch(rng, B, n, R, D, L, Vq, n_ws, A)
    if "ew" in heads:
        batch = ER.add_enwiki_fields(rng, batch, CTX["n_ctx"], CTX["Lc"])

    def engine():
        e = PT.PretrainEngine(n=n, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=n_ws, params=p, heads=heads, n_ctx=nc, noc=noc,
                              adapt=adapt, deterministic=True, precision=precision)
        assert e.ln_shared == ln_shared
        return e
    return PT, p, batch, engine


def _u8_tensors(obj, seen=None):
    """uint8 tensors reachable from an engine's attributes, the workspace (a byte buffer) aside"""
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return []
    seen.add(id(obj))
    if torch.is_tensor(obj):
        return [obj] if obj.dtype == torch.uint8 else []
    if isinstance(obj, dict):
        return sum((_u8_tensors(v, seen) for v in obj.values()), [])
    if isinstance(obj, (list, tuple)):
        return sum((_u8_tensors(v, seen) for v in obj), [])
    return []


def _engine_u8(eng):
    return sum((_u8_tensors(v) for k, v in vars(eng).items() if k != "workspace"), [])


def _tape_tensors(eng):
    out = []
    for k in sorted(eng._tape["kinds"]):
        kt = eng._tape["kinds"][k]
        out += [kt["att"], kt["pooled"]]
        for task in sorted(t for t in kt if t not in ("att", "pooled")):
            out += [kt[task][z] for z in sorted(kt[task])]
    return out


def _steps_equal(model, cfg, ln_shared=True, sort=False, rows=None, steps=(3, 4), precision="f32"):
    """two train steps: X on make_keep_masks(B, seed, step), Y with dropout=(seed, step).  rows=(lo, hi, global): both on
    that shard of the batch, with the stream positions of the global rows"""
    PT, p, batch, engine = _model_case(model, cfg, ln_shared, precision=precision)
    if rows is not None:
        lo, hi, Bg = rows
        batch = {k: v[lo:hi] for k, v in batch.items()}
    B = batch["image_ft"].shape[0]
    X, Y = engine(), engine()
    assert Y._abi == MODELS[model][3]
    dbs = []
    for _ in range(2):       # one device batch per engine: the engines cache converted tensors on it
        db = {k: dev(v) for k, v in batch.items()}
        if sort:
            db.update({k: v for k, v in PT.add_length_sort(dict(batch)).items() if k.endswith("/sort")})
        dbs.append(db)
    for step in steps:
        if rows is None:
            masks, dropout = X.make_keep_masks(B, SEED, step), (SEED, step)
        else:
            masks, dropout = X.make_keep_masks(B, SEED, step, row_offset=lo, global_rows=Bg), (SEED, step, lo, Bg)
        X.train_step(dbs[0], masks, 1e-3)
        Y.train_step(dbs[1], None, 1e-3, dropout=dropout)
        torch.cuda.synchronize()
        assert torch.isfinite(Y.grad_flat).all()
        for n in X.train_names:
            assert torch.equal(X.grads[n], Y.grads[n]), (step, n)
        assert torch.equal(X.grad_flat, Y.grad_flat), step
        for i, (a, b) in enumerate(zip(_tape_tensors(X), _tape_tensors(Y))):
            assert torch.equal(a, b), (step, "tape", i)
        rx, ry = X.fetch_report(), Y.fetch_report()
        assert rx == ry and np.isfinite(list(ry.values())).all(), step
    for n in X.params:
        assert torch.equal(X.params[n], Y.params[n]), n
    assert torch.equal(X.train_flat, Y.train_flat) and torch.equal(X.m_flat, Y.m_flat) and torch.equal(X.v_flat, Y.v_flat)
    assert not _engine_u8(Y) and len(_engine_u8(X)) >= 6       # the seeded engine holds no mask tensor
    return PT, X, Y, dbs, batch


@pytest.mark.parametrize("cfg,sort,ln_shared", [(TOY, False, True), (TOY, True, False), (MID, True, True), (MID, False, False)],
                         ids=["toy-as-given-shared", "toy-sorted-per-site", "mid-sorted-shared", "mid-as-given-per-site"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_seeded_step_equals_explicit_step(model, cfg, sort, ln_shared):
    _steps_equal(model, cfg, ln_shared, sort)


@pytest.mark.parametrize("model,cfg", [("cfg5", WIDE), ("adapt", WIDE_ADAPT)], ids=["cfg5", "adapt"])
def test_seeded_step_equals_explicit_step_h1024(model, cfg):
    """the per-memory rep-5 attention kernels (forward and fast backward, D 2048 and the 1024-wide memory) inside a step"""
    _steps_equal(model, cfg)


@pytest.mark.parametrize("model", ["cfg5", "noc_bf_ew", "adapt"])
def test_seeded_step_equals_explicit_step_bf16(model):
    """precision="bf16" routes GEMMs only: every dropout site is the f32 engine's, seeded or explicit"""
    _steps_equal(model, MID, sort=True, precision="bf16")


def test_dropout_does_something_and_none_is_todays_forward():
    PT, X, Y, dbs, batch = _steps_equal("cfg5", TOY, steps=(3,))
    Y.forward(dbs[1], None, want_dz=False, dropout=(SEED, 5))
    with_dropout = [t.clone() for t in _tape_tensors(Y)]
    X.forward(dbs[0], None, want_dz=False)
    Y.forward(dbs[1], None, want_dz=False, dropout=None)
    torch.cuda.synchronize()
    for a, b in zip(_tape_tensors(X), _tape_tensors(Y)):
        assert torch.equal(a, b)
    assert not all(torch.equal(a, b) for a, b in zip(with_dropout, _tape_tensors(Y)))


@pytest.mark.parametrize("model", ["cfg5", "noc_bf_ew"])
def test_shard_draws_the_bits_of_the_whole_batch(model):
    """rows 8..15 of a 16-image batch: dropout=(seed, step, 8, 16) is the explicit step on make_keep_masks(8, seed, step,
    row_offset=8, global_rows=16)"""
    PT, X, Y, dbs, batch = _steps_equal(model, MID, rows=(8, 16, 16))
    # ... and those are other bits than the shard's own rows 0..7 would draw
    Y.forward(dbs[1], None, want_dz=False, dropout=(SEED, 9, 8, 16))
    a = [t.clone() for t in _tape_tensors(Y)]
    Y.forward(dbs[1], None, want_dz=False, dropout=(SEED, 9), row_offset=8, global_rows=16)      # the keyword form
    assert all(torch.equal(x, y) for x, y in zip(a, _tape_tensors(Y)))
    Y.forward(dbs[1], None, want_dz=False, dropout=(SEED, 9, 0, 16))
    assert not all(torch.equal(x, y) for x, y in zip(a, _tape_tensors(Y)))


def test_masks_together_with_dropout_raise():
    PT, p, batch, engine = _model_case("cfg5", TOY)
    eng = engine()
    db = {k: dev(v) for k, v in batch.items()}
    masks = eng.make_keep_masks(TOY["B"], SEED, 0)
    with pytest.raises(ValueError, match="mutually exclusive"):
        eng.forward(db, masks, dropout=(SEED, 0))
    with pytest.raises(ValueError, match="mutually exclusive"):
        eng.train_step(db, masks, 1e-3, dropout=(SEED, 0))
    with pytest.raises(ValueError, match="seed, step"):
        eng.forward(db, None, dropout=(SEED, 0, 0))


def test_c_abi_refuses_a_seeded_site_that_also_has_a_mask():
    """on the engine's own structs: the forward with every site seeded AND the explicit masks bound"""
    import ctypes as C
    L = _lib()
    PT, p, batch, engine = _model_case("noc_bf_ws", TOY)
    eng = engine()
    db = {k: dev(v) for k, v in batch.items()}
    eng.forward(db, eng.make_keep_masks(TOY["B"], SEED, 0))
    ks = eng._keep_struct(TOY["B"], (SEED, 0))
    for site, bit in L.PT_KEEP_SITE.items():
        if site == "ew_joint":
            continue        # this model has no enwiki head: its ew mask pointer is NULL
        one = L.PtKeep(keep_seed=SEED, seeded=bit)
        rc = eng.lib.vqa_pretrain_noc_forward_ex(C.byref(eng.dims), C.byref(eng._p_struct), C.byref(eng._bs),
                                                 C.c_void_p(eng.workspace.data_ptr()), eng.workspace.numel(), 1, eng._stream(),
                                                 C.byref(one))
        assert rc == -1, (site, rc)
    assert ks.seeded == 1 | 2 | 4 | 16
    bad = L.PtKeep(keep_seed=SEED, seeded=64)
    assert eng.lib.vqa_pretrain_noc_forward_ex(C.byref(eng.dims), C.byref(eng._p_struct), C.byref(eng._bs),
                                               C.c_void_p(eng.workspace.data_ptr()), eng.workspace.numel(), 1, eng._stream(),
                                               C.byref(bad)) == -1
    # an offset that is no multiple of 4: VQA_ERR_ALIGN from the keep source, before the site's kernel
    eng.forward(db, None)
    odd = eng._keep_struct(TOY["B"], (SEED, 0))
    odd.att_off[0] += 2
    rc = eng.lib.vqa_pretrain_noc_forward_ex(C.byref(eng.dims), C.byref(eng._p_struct), C.byref(eng._bs),
                                             C.c_void_p(eng.workspace.data_ptr()), eng.workspace.numel(), 1, eng._stream(),
                                             C.byref(odd))
    assert rc != 0 and b"align" in eng.lib.vqa_hot_error_string(rc)


def _trainer(tmp_path, inline, steps=3, Vq=60, A=30):
    """a PretrainTrainer on the synthetic dataset (cfg-5, batch 8, H 1024, R 36, D 64), deterministic so that two runs can
    be compared bit for bit"""
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV, pretrain_trainer as PTT
    data = DV.synthetic_dataset(40, Vq, 12, A, R=36, D=64, max_len=6, seed=5)
    ds = {"train": DV.Dataset(split="train", data=data, seed=1), "val": DV.Dataset(split="val", data=data, seed=2)}
    cfg = PTT.build_parser().parse_args(["--batch_size", "8", "--max_train_iter", str(steps), "--learning_rate", "0.002",
                                         "--model_type", "vlmap_bf_or_wordset_withatt_sp", "--features_on_device", "1",
                                         "--input_workers", "0", "--input_prefetch", "0", "--expand_depth", "true"] +
                                        (["--inline_dropout"] if inline else []))
    cfg.data_cfg = ds["train"].get_config()
    cfg.vocab = {"vocab": ["w%d" % i for i in range(Vq)], "dict": {"w%d" % i: i for i in range(Vq)}}
    cfg.answer_dict, cfg.ws_dict = data["answer_dict"], data["ws_dict"]
    cfg.synthetic, cfg.deterministic, cfg.train_dir = 1, 1, str(tmp_path / ("pre_inline_%d" % inline))
    return PTT.Trainer(cfg, ds)


def test_trainer_with_inline_dropout_reproduces_the_explicit_run(tmp_path):
    from vqa_transfer_externaldata_amd import pretrain_trainer as PTT
    losses = {}
    for inline in (False, True):
        t = _trainer(tmp_path, inline)
        losses[inline] = [float(t.run_train_step(False)[2]) for _ in range(3)]
        assert t.model.engine.deterministic and bool(_engine_u8(t.model.engine)) != inline
    assert losses[True] == losses[False] and np.isfinite(losses[True]).all()
    assert len(set(losses[True])) == 3
    assert PTT.build_parser().parse_args(["--inline_dropout"]).inline_dropout
    assert not PTT.build_parser().parse_args([]).inline_dropout
