"""The region features at rest as bf16 in the bf16 pre-training steps: PretrainEngine(precision="bf16", features="bf16")
(VQA_FLAG_BF16_FEATURES in vqa_pretrain_dims_t.flags; vqa_pretrain_*, _ext_*, _noc_* and _adapt_*).

The criterion everywhere is torch.equal between two engines built from the same parameters: Y runs on t16 = the features
rounded to bf16, X runs precision="bf16" on t16.float() (tests/pretrain_bf16_features_util.py).  No tolerance: rounding is
idempotent and no sum changes its order.  X is pinned to the float64 reference by tests/test_gpu_pretrain_bf16.py.

The several-queries-per-memory attention kernels have no op-level entry point for a bf16 memory, so each of them is
reached through the step, once per keep policy, at the smallest shape that selects it (the shape table in the helper file),
and compared on the named intermediates <kind>/att, <kind>/pooled, d_v, d_qv, part_dw, part_db (adapt: va_pre and v_adapt's
weight gradient), every gradient, grad_flat, the parameters and both Adam slots after two train steps, and the report.

The C-level refusal at the bottom needs no GPU and is not marked."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pretrain_bf16_features_util as U

gpu = pytest.mark.gpu


def _pair(model, shape, keep, tables=False, ln_shared=True):
    ex, x = U.run(model, shape, keep, tables, ln_shared, bf16=False)
    ey, y = U.run(model, shape, keep, tables, ln_shared, bf16=True)
    assert (ex.features, ey.features) == ("f32", "bf16") and ex.precision == ey.precision == "bf16"
    base = lambda e: e.dims.base if e.ext else e.dims
    assert base(ex).flags & 24 == 8 and base(ey).flags & 24 == 24
    assert ex.workspace.numel() == ey.workspace.numel()                      # image_ft is an input: no layout changes
    assert {k: tuple(v.shape) for k, v in ex.state_dict().items()} == {k: tuple(v.shape) for k, v in ey.state_dict().items()}
    U.assert_pair_equal(x, y, "%s %s %s%s" % (model, shape, keep, " tables" if tables else ""))
    return ey


# ------------------------------------------------------------------------------------------------ 1. the attention routes
ROUTE_SHAPES = ("full", "full_r3", "full_r7", "full_r40", "h256", "toy", "medium", "n7")


@gpu
@pytest.mark.parametrize("keep", U.KEEPS)
@pytest.mark.parametrize("shape", ROUTE_SHAPES)
def test_every_attention_route_in_every_keep_policy(shape, keep):
    """cfg-5 with a direct bf16 image_ft.  full / full_r3 / full_r7 / full_r40: the per-memory forward and the fast backward
    <5> (R below REP_PF, one partial pooling batch, the bound); h256: the per-memory forward at H 256, D 4096 with the
    generic backward <5>; toy, medium: generic forward and generic backward <5>; n7: generic backward <8>."""
    ey = _pair("cfg5", shape, keep)
    if keep == "seeded":
        assert ey._ks is not None and ey._ks.seeded


@gpu
@pytest.mark.parametrize("keep", U.KEEPS)
@pytest.mark.parametrize("fast", [0, 3])
def test_attn_set_fast_settings(fast, keep):
    """vqa_attn_set_fast(0): all generic; (3): the per-query fast forward with rep 5 (and the fast backward <5>)"""
    from vqa_transfer_externaldata_amd import _lib
    lib = _lib.load()
    try:
        assert lib.vqa_attn_set_fast(fast) == 0
        _pair("cfg5", "full", keep)
    finally:
        lib.vqa_attn_set_fast(1)


# ------------------------------------------------------------------------------------------------ 2. the engine families
FAMILY_CASES = [(m, s, k) for m in ("enwiki", "noc", "adapt") for s, k in (("medium", "masks"), ("full", "seeded"))] + \
               [("cfg5", "medium", "masks"), ("cfg5", "full", "seeded"), ("adapt", "medium", "none")]


@gpu
@pytest.mark.parametrize("model,shape,keep", FAMILY_CASES, ids=["%s-%s-%s" % c for c in FAMILY_CASES])
def test_every_family_on_bound_tables(model, shape, keep):
    """bound tables and image_idx with a repeated image: vqa_gather_features_bf16 feeds the step.  adapt: the pooled memory
    is the f32 v_adapt, the features are the left operand of v_adapt's forward and dW products (vqa_gemm_bf16_a16)."""
    ey = _pair(model, shape, keep, tables=True)
    assert ey._tables[0].dtype == torch.bfloat16 and ey._keepalive[2][0].dtype == torch.bfloat16        # table and gathered rows
    if model == "adapt":
        assert float(ey.grads["v_adapt/fc/weights"].abs().max()) > 0


@gpu
def test_adapt_with_one_layernorm_per_call_site():
    _pair("adapt", "medium", "masks", ln_shared=False)


@gpu
@pytest.mark.parametrize("model", ["enwiki", "noc", "adapt"])
def test_every_family_on_a_direct_bf16_image_ft(model):
    _pair(model, "medium", "seeded")


# ------------------------------------------------------------------------------------------------ 3. the default
@gpu
@pytest.mark.parametrize("model", U.MODELS)
def test_features_f32_is_bitwise_the_engine_without_the_argument(model):
    res = []
    for kw in ({"precision": "bf16"}, {"precision": "bf16", "features": "f32"}, {}, {"features": "f32"}):
        eng, out = U.run(model, "medium", "masks", bf16=False, engine_kw=kw)
        assert eng.features == "f32" and not eng._flags() & 16
        res.append(out)
    U.assert_pair_equal(res[0], res[1], model + " bf16")
    U.assert_pair_equal(res[2], res[3], model + " f32")
    assert not torch.equal(res[0]["grad_flat"], res[2]["grad_flat"])


# ------------------------------------------------------------------------------------------------ 4. refusals
@gpu
def test_engine_refusals():
    with pytest.raises(ValueError, match="precision='bf16'"):
        U.engine("cfg5", "toy", features="bf16")
    with pytest.raises(ValueError, match="precision='bf16'"):
        U.engine("cfg5", "toy", precision="f32", features="bf16")
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError, match="features"):
            U.engine("cfg5", "toy", precision="bf16", features=bad)


@gpu
def test_table_and_batch_refusals():
    PT, eng = U.engine("cfg5", "toy", precision="bf16", features="bf16")
    ekw, p, batch, masks, d = U.make_case("cfg5", "toy")
    table, spat, nbox, idx = U.make_tables(d)
    t32 = U.dev(table)
    good = t32.to(torch.bfloat16)
    for what, bad in (("f32", t32), ("half", t32.half()), ("host", good.cpu()), ("numpy", table),
                      ("mis-shaped", good[:, :, :-4].contiguous()), ("2-d", good.view(-1, d["D"])),
                      ("not contiguous", good.transpose(0, 1).contiguous().transpose(0, 1))):
        with pytest.raises(ValueError, match="features_to_bf16"):
            eng.bind_tables(bad, spat, nbox)
        assert getattr(eng, "_tables", None) is None, what              # nothing was bound, nothing converted
    eng.bind_tables(good, spat, nbox)
    assert eng._tables[0].data_ptr() == good.data_ptr()                  # taken as it is
    # a batch that carries image_ft itself
    PT, eng = U.engine("cfg5", "toy", precision="bf16", features="bf16")
    db = {k: U.dev(v) for k, v in batch.items()}
    for bad in (db["image_ft"], db["image_ft"].half(), batch["image_ft"], db["image_ft"].to(torch.bfloat16).cpu(),
                db["image_ft"].to(torch.bfloat16)[:, :, :-4].contiguous()):
        with pytest.raises(ValueError, match="features_to_bf16"):
            eng.forward(dict(db, image_ft=bad), None)
    eng.forward(dict(db, image_ft=db["image_ft"].to(torch.bfloat16)), None)
    torch.cuda.synchronize()
    assert np.isfinite(list(eng.fetch_report().values())).all()


def _flag_dims(_lib, flags, ext):
    d = _lib.PtDims(B=2, n=5, R=36, D=2048, H=1024, W=300, A=100, Vq=50, n_ws=20, L=6, flags=flags, keep_att=0.8,
                    keep_joint=0.5)
    return _lib.PtExtDims(base=d, heads=_lib.PT_HEAD_BF | _lib.PT_HEAD_WS, Lc=0, n_ctx=0) if ext else d


def test_the_flag_without_bf16_gemm_is_err_arg_in_every_family():
    """Host only (no launch, no GPU): VQA_FLAG_BF16_FEATURES without VQA_FLAG_BF16_GEMM makes the workspace query and the
    tensor query of each of the four families return VQA_ERR_ARG, forward and backward_phases (the _ex forms too) return it
    before they look at any pointer; with both flags the queries answer, and the layout is that of VQA_FLAG_BF16_GEMM."""
    import __graft_entry__ as g
    g.build()
    from vqa_transfer_externaldata_amd import _lib
    lib = _lib.load()
    ERR_ARG = -1
    G, F = _lib.FLAG_BF16_GEMM, _lib.FLAG_BF16_FEATURES
    assert (G, F) == (8, 16)
    params = {"vqa_pretrain_": _lib.PtParams, "vqa_pretrain_ext_": _lib.PtExtParams, "vqa_pretrain_noc_": _lib.PtNocParams,
              "vqa_pretrain_adapt_": _lib.PtAdaptParams}
    batches = {"vqa_pretrain_": _lib.PtBatch, "vqa_pretrain_ext_": _lib.PtExtBatch, "vqa_pretrain_noc_": _lib.PtNocBatch,
               "vqa_pretrain_adapt_": _lib.PtExtBatch}
    for abi in params:
        ext = abi != "vqa_pretrain_"
        wq, tq = getattr(lib, abi + "workspace_bytes"), getattr(lib, abi + "tensor")
        off, cnt = C.c_int64(), C.c_int64()
        for shared in (0, _lib.FLAG_SHARED_LN):
            bad = _flag_dims(_lib, F | shared, ext)
            assert wq(C.byref(bad)) == ERR_ARG, abi
            assert tq(C.byref(bad), b"obj/att", C.byref(off), C.byref(cnt)) == ERR_ARG, abi
            P, Gd, bt, ws = params[abi](), params[abi](), batches[abi](), (C.c_char * 64)()
            ks = _lib.PtKeep()
            st = None
            assert getattr(lib, abi + "forward")(C.byref(bad), C.byref(P), C.byref(bt), ws, 64, 1, st) == ERR_ARG, abi
            assert getattr(lib, abi + "forward_ex")(C.byref(bad), C.byref(P), C.byref(bt), ws, 64, 1, st, C.byref(ks)) == ERR_ARG
            assert getattr(lib, abi + "backward")(C.byref(bad), C.byref(P), C.byref(Gd), C.byref(bt), ws, 64, None, st) == ERR_ARG
            assert getattr(lib, abi + "backward_phases")(C.byref(bad), C.byref(P), C.byref(Gd), C.byref(bt), ws, 64, None, 1,
                                                         st) == ERR_ARG
            assert getattr(lib, abi + "backward_phases_ex")(C.byref(bad), C.byref(P), C.byref(Gd), C.byref(bt), ws, 64, None, 1,
                                                            st, C.byref(ks)) == ERR_ARG
            size = {}
            for flags in (G, G | F):
                ok = _flag_dims(_lib, flags | shared, ext)
                assert tq(C.byref(ok), b"obj/att", C.byref(off), C.byref(cnt)) == 0
                size[flags] = (int(wq(C.byref(ok))), off.value, cnt.value)
            assert size[G] == size[G | F] and size[G][0] > 0, (abi, size)


# ------------------------------------------------------------------------------------------------ 5. the trainer
@gpu
def test_trainer_with_bf16_features_lowers_the_loss_and_its_checkpoint_loads_in_an_f32_engine(tmp_path):
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV, pretrain as PT, pretrain_trainer as PTT
    assert PTT.build_parser().parse_args([]).features == "f32"
    assert PTT.build_parser().parse_args(["--precision", "bf16", "--features", "bf16"]).features == "bf16"
    with pytest.raises(SystemExit):
        PTT.build_parser().parse_args(["--features", "fp16"])
    A, Vq = 30, 60
    data = DV.synthetic_dataset(40, Vq, 12, A, R=36, D=64, max_len=6, seed=5)
    ds = {"train": DV.Dataset(split="train", data=data, seed=1), "val": DV.Dataset(split="val", data=data, seed=2)}
    cfg = PTT.build_parser().parse_args(["--batch_size", "8", "--max_train_iter", "10", "--learning_rate", "0.002",
                                         "--features_on_device", "1", "--input_workers", "0", "--input_prefetch", "0",
                                         "--precision", "bf16", "--features", "bf16", "--inline_dropout"])
    cfg.data_cfg = ds["train"].get_config()
    cfg.vocab = {"vocab": ["w%d" % i for i in range(Vq)], "dict": {"w%d" % i: i for i in range(Vq)}}
    cfg.answer_dict, cfg.ws_dict = data["answer_dict"], data["ws_dict"]
    cfg.synthetic, cfg.train_dir = 1, str(tmp_path / "pre_bf16_features")
    t = PTT.Trainer(cfg, ds)
    eng = t.model.engine
    assert eng.precision == "bf16" and eng.features == "bf16" and eng._flags() & 24 == 24
    assert eng._tables[0].dtype == torch.bfloat16 and eng._tables[0].is_cuda       # rounded once, bound as bf16
    losses = []
    for _ in range(10):
        step, _, loss, report, _ = t.run_train_step(False)
        losses.append(loss)
    print("trainer --precision bf16 --features bf16 --inline_dropout, total_loss per step:", ["%.4f" % v for v in losses])
    assert eng._ks is not None and eng._ks.seeded                                   # the keep bits were drawn in the kernels
    assert np.isfinite(losses).all() and np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    sd = torch.load(t.save_checkpoint())
    assert all(v.dtype in (torch.float32, torch.int64) for v in sd.values())
    zeros = {k: np.zeros(shp, np.float32) for k, shp in eng.shapes.items()}
    e32 = PT.PretrainEngine(n=eng.n, R=eng.R, D=eng.D, H=eng.H, W=eng.W, A=eng.A, Vq=eng.Vq, n_ws=eng.n_ws, params=zeros)
    assert (e32.precision, e32.features) == ("f32", "f32") and not e32._flags() & 24
    e32.load_state_dict(sd)
    assert e32.step_count == 10
    for k, v in eng.params.items():
        assert torch.equal(v, e32.params[k]), k
    assert sorted(e32.state_dict()) == sorted(eng.state_dict())
