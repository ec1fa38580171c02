"""GPU parity of the enwiki-context pre-training models (vlmap_memft/model_vlmap_bf_or_wordset_enwiki_withatt_sp.py and
model_vlmap_bf_enwiki_withatt_sp.py) against the float64 reference of tests/pretrain_enwiki_ref.py: report, logits, every
gradient and the slice sum of squares; the trainer, the export bridge into the VQA trainer, data parallelism.

The C entry points exercised here: vqa_pretrain_ext_workspace_bytes, vqa_pretrain_ext_tensor, vqa_pretrain_ext_report_key,
vqa_pretrain_ext_forward, vqa_pretrain_ext_backward, vqa_pretrain_ext_backward_phases (structs vqa_pretrain_ext_dims_t,
vqa_pretrain_ext_params_t, vqa_pretrain_ext_batch_t, vqa_pretrain_ctx_kind_t, vqa_pt_fc6_t; head bits VQA_PT_HEAD_BF,
VQA_PT_HEAD_WS, VQA_PT_HEAD_EW)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

from oracle import pretrain_oracle as PO
from tests import pretrain_enwiki_ref as ER

pytestmark = pytest.mark.gpu

TYPES = {"vlmap_bf_or_wordset_enwiki_withatt_sp": ("bf", "ws", "ew"), "vlmap_bf_enwiki_withatt_sp": ("bf", "ew")}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to64(d):
    return {k: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in d.items()}


def _setup(seed, heads, B, n, R, D, H, L, W, Vq, n_ws, A, n_ctx, Lc, ln_shared=True, deterministic=False):
    from vqa_transfer_externaldata_amd import pretrain as PT
    rng = np.random.default_rng(seed)
    p = ER.init_params(rng, Vq, n_ws, A, W=W, D=D, H=H, ln_shared=ln_shared, heads=heads, n_ctx=n_ctx)
    batch = ER.add_enwiki_fields(rng, PO.make_batch(rng, B, n, R, D, L, Vq, n_ws, A), n_ctx, Lc)
    masks = ER.add_enwiki_masks(rng, PO.make_masks(rng, B, n, R, H), B, n, H)
    eng = PT.PretrainEngine(n=n, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=n_ws, params=p, heads=heads, n_ctx=n_ctx,
                            deterministic=deterministic)
    assert eng.ln_shared == ln_shared and eng.ext
    db = {k: dev(v) for k, v in batch.items()}
    dm = {k: dev(v.astype(np.uint8)) for k, v in masks.items()}
    return PT, eng, p, batch, masks, db, dm


def hip_relu_gates(eng, B, heads):
    n, R, H = eng.n, eng.R, eng.H
    g = {}
    for k in PO.KINDS:
        g[k + "/v"] = (eng.tensor(k + "/v").view(B, R, H) > 0).cpu().numpy()
        g[k + "/qv"] = (eng.tensor(k + "/qv").view(B, n, H) > 0).cpu().numpy()
        for hd in heads:
            for t, w in (("vl", H), ("ll", H), ("j", 2 * H)):
                g["%s/%s/%s" % (k, hd, t)] = (eng.tensor("%s/%s/%s" % (k, hd, t)).view(B, n, w) > 0).cpu().numpy()
    return g


SMALL = [dict(B=3, n=5, R=6, D=16, H=8, L=4, W=12, Vq=20, n_ws=7, A=12, n_ctx=15, Lc=7),
         dict(B=16, n=5, R=36, D=256, H=128, L=10, W=300, Vq=200, n_ws=50, A=400, n_ctx=90, Lc=7)]


@pytest.mark.parametrize("ln_shared", [True, False])
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("model_type", sorted(TYPES))
@pytest.mark.parametrize("cfg", SMALL)
def test_forward_backward_match_f64_reference(cfg, model_type, sort, ln_shared):
    heads = TYPES[model_type]
    PT, eng, p, batch, masks, db, dm = _setup(5, heads, ln_shared=ln_shared, **cfg)
    if sort:       # captions and contexts in length order, the recurrences on the live prefix: same results
        db.update({k: v for k, v in PT.add_length_sort(dict(batch)).items() if k.endswith("/sort")})
        assert "enwiki_context/sort" in db
    eng.forward(db, dm)
    eng.backward()
    torch.cuda.synchronize()
    rep = eng.fetch_report()
    total, report, mid = ER.forward(to64(p), to64(batch), to64(masks), cfg["n"], heads)
    assert list(rep) == ER.report_keys(heads) and len(rep) == (19 if "ws" in heads else 13)
    for k in report:
        assert abs(rep[k] - report[k]) <= 2e-4 * max(1.0, abs(report[k])), (k, rep[k], report[k])
    for k in PO.KINDS:
        for hd in heads:
            z = eng._tape["kinds"][k][ER.TASK[hd]]["z"].cpu().numpy().reshape(mid["%s/%s_logit" % (k, hd)].shape)
            assert np.abs(z - mid["%s/%s_logit" % (k, hd)]).max() < 1e-3, (k, hd)
    _, _, grads, slices = ER.torch_loss_and_grads(to64(p), to64(batch), to64(masks), cfg["n"], heads)
    assert sorted(eng.train_names) == sorted(k for k in p if k not in PT.NO_GRAD_VARS)
    for name in eng.train_names:
        g = eng.grads[name].cpu().numpy().astype(np.float64)
        if name.endswith("score/fc/biases"):
            assert np.abs(g).max() < 1e-5
            continue
        if name == "wordset_map/learn" and "ws" not in heads:
            assert not g.any()                         # exists in bf_enwiki, gets no gradient
            continue
        sc = max(np.abs(grads[name]).max(), 1e-12)
        assert np.abs(g - grads[name]).max() <= 1e-3 * sc + 1e-8, (name, np.abs(g - grads[name]).max(), sc)
    sq = sum(float((v ** 2).sum()) for v in slices.values())
    assert abs(float(eng.grad_flat[eng.n_train]) - sq) <= 1e-3 * sq + 1e-12


def test_full_size_bf_or_wordset_enwiki_bs512_matches_f64():
    """What TF builds (shared LayerNorms) at BASELINE size: B 512, n 5, R 36, D 2048, H 1024, captions <= 10 tokens,
    contexts <= 7, A 4000 -- the bars of test_full_size_cfg5_bs512_matches_oracle_f64."""
    heads = TYPES["vlmap_bf_or_wordset_enwiki_withatt_sp"]
    cfg = dict(B=512, n=5, R=36, D=2048, H=1024, L=10, W=300, Vq=5000, n_ws=2000, A=4000, n_ctx=3000, Lc=7)
    PT, eng, p, batch, masks, db, dm = _setup(9, heads, ln_shared=True, **cfg)
    db.update({k: v for k, v in PT.add_length_sort(dict(batch)).items() if k.endswith("/sort")})
    eng.forward(db, dm)
    eng.backward()
    torch.cuda.synchronize()
    rep = eng.fetch_report()
    p64, b64, m64 = to64(p), to64(batch), to64(masks)
    total, report, mid = ER.forward(p64, b64, m64, cfg["n"], heads)
    for k in report:
        assert abs(rep[k] - report[k]) <= 2e-4 * max(1.0, abs(report[k])), (k, rep[k], report[k])
    for k in PO.KINDS:
        for hd in heads:
            want = mid["%s/%s_logit" % (k, hd)]
            z = eng._tape["kinds"][k][ER.TASK[hd]]["z"].cpu().numpy().reshape(want.shape)
            assert np.abs(z - want).max() < 1e-3, (k, hd, np.abs(z - want).max())
    del mid
    hip = {name: eng.grads[name].cpu().numpy().astype(np.float64) for name in eng.train_names}
    gates = hip_relu_gates(eng, cfg["B"], heads)
    _, _, gc, slices = ER.torch_loss_and_grads(p64, b64, m64, cfg["n"], heads, gates=gates)
    worst = {}
    for name in eng.train_names:
        if name.endswith("score/fc/biases"):
            assert np.abs(hip[name]).max() < 1e-5
            continue
        worst[name] = np.abs(hip[name] - gc[name]).max() / max(np.abs(gc[name]).max(), 1e-30)
    bad = {k: v for k, v in worst.items() if v > 5e-4}
    assert not bad, bad
    sq = sum(float((v ** 2).sum()) for v in slices.values())
    assert abs(float(eng.grad_flat[eng.n_train]) - sq) <= 1e-3 * sq + 1e-12
    cap = {}
    _, _, gu, _ = ER.torch_loss_and_grads(p64, b64, m64, cfg["n"], heads, capture=cap)
    sites = [s for s in ER.relu_sites(heads) if not s.endswith("/j")]
    flips = sum(int((cap[s] != gates[s]).sum()) for s in sites)
    assert flips <= 1e-5 * sum(cap[s].size for s in sites), flips
    for name in eng.train_names:
        if name.endswith("score/fc/biases"):
            continue
        fro = np.linalg.norm(hip[name] - gu[name]) / max(np.linalg.norm(gu[name]), 1e-30)
        assert fro <= 5e-3, (name, fro)


def test_c_abi_report_keys_workspace_and_phases():
    """vqa_pretrain_ext_report_key per head set, the workspace / named tensors, and vqa_pretrain_ext_backward_phases
    1, 2, 4, 8 one by one == vqa_pretrain_ext_backward bit for bit (deterministic), every bucket written by its phase."""
    from vqa_transfer_externaldata_amd import _lib
    lib = _lib.load()
    for heads, mask in ((("bf", "ws", "ew"), 7), (("bf", "ew"), 5), (("bf", "ws"), 3)):
        keys = []
        while lib.vqa_pretrain_ext_report_key(mask, len(keys)) is not None:
            keys.append(lib.vqa_pretrain_ext_report_key(mask, len(keys)).decode())
        assert keys == ER.report_keys(heads)
    assert [lib.vqa_pretrain_ext_report_key(3, i).decode() for i in range(13)] == \
        [lib.vqa_pretrain_report_key(i).decode() for i in range(13)]
    assert lib.vqa_pretrain_ext_report_key(2, 0) is None          # the blank-fill head is required
    cfg = dict(SMALL[0])
    heads = TYPES["vlmap_bf_or_wordset_enwiki_withatt_sp"]
    out = []
    for phased in (False, True):
        PT, eng, p, batch, masks, db, dm = _setup(11, heads, deterministic=True, **cfg)
        eng.forward(db, dm)
        d = eng.dims
        assert isinstance(d, _lib.PtExtDims) and d.heads == (_lib.PT_HEAD_BF | _lib.PT_HEAD_WS | _lib.PT_HEAD_EW)
        assert lib.vqa_pretrain_ext_workspace_bytes(C.byref(d)) == eng.workspace.numel()
        assert eng.tensor("E/ctx_s", torch.int32).numel() == 2 * cfg["B"] * cfg["n"] * cfg["Lc"]
        bad = _lib.PtExtDims(base=d.base, heads=_lib.PT_HEAD_EW, Lc=d.Lc, n_ctx=d.n_ctx)
        assert lib.vqa_pretrain_ext_workspace_bytes(C.byref(bad)) < 0
        if phased:
            eng.grad_flat.fill_(float("nan"))
            b0, b1, b2, b3 = eng._bounds[:4]
            for ph, (lo, hi) in ((1, (b2, b3)), (2, (b1, b2)), (4, (b0, b1))):
                eng._backward_phases(ph)
                torch.cuda.synchronize()
                used = torch.zeros(eng.n_train, dtype=torch.bool)
                for k, (o, cnt) in eng._tab.items():
                    used[o:o + cnt] = True
                assert not torch.isnan(eng.grad_flat[lo:hi].cpu()[used[lo:hi]]).any(), ph
            eng._backward_phases(8)
        else:
            tail = eng.grad_flat[eng.n_train:]
            _lib.check(lib.vqa_pretrain_ext_backward(C.byref(d), C.byref(eng._p_struct), C.byref(eng._g_struct),
                                                     C.byref(eng._bs), C.c_void_p(eng.workspace.data_ptr()),
                                                     eng.workspace.numel(), C.c_void_p(tail.data_ptr()), eng._stream()),
                       "vqa_pretrain_ext_backward")
        torch.cuda.synchronize()
        g = eng.grad_flat.cpu().numpy().copy()
        mask = np.zeros(eng.n_train + 4, bool)
        for k, (o, cnt) in eng._tab.items():
            mask[o:o + cnt] = True
        mask[eng.n_train] = True
        out.append(g[mask])
    np.testing.assert_array_equal(out[0], out[1])
    names = eng.train_names
    assert names[:3] == ["wordset_map/learn", "L_GloVe/embed_map", "enwiki_map/learn"]
    assert names[3].startswith("encode_L_blank/") and names[7].startswith("encode_L_enwiki/")


def test_keep_masks_of_the_cfg5_streams_are_unchanged():
    """the enwiki heads' joint masks come from a disjoint counter range: att / bf_joint / ws_joint bits for (seed, step,
    global row) are those of the cfg-5 engine, data-parallel shards included"""
    from vqa_transfer_externaldata_amd import pretrain as PT
    cfg = dict(n=5, R=6, D=16, H=8, W=12, A=12, Vq=20, n_ws=7)
    rng = np.random.default_rng(1)
    c5 = PT.PretrainEngine(params=PO.init_params(rng, 20, 7, 12, W=12, D=16, H=8), **cfg)
    ew = PT.PretrainEngine(params=ER.init_params(rng, 20, 7, 12, W=12, D=16, H=8, n_ctx=15), heads=("bf", "ws", "ew"),
                           n_ctx=15, **cfg)
    for step, lo, B, Bg in ((0, 0, 4, None), (3, 2, 3, 7)):
        a = c5.make_keep_masks(B, 123, step, row_offset=lo, global_rows=Bg)
        b = ew.make_keep_masks(B, 123, step, row_offset=lo, global_rows=Bg)
        assert sorted(b) == sorted(list(a) + ["obj/ew_joint", "attr/ew_joint"])
        for k in a:
            assert torch.equal(a[k], b[k]), k
        for k in ("obj/ew_joint", "attr/ew_joint"):
            keep = b[k].float().mean().item()
            assert 0.3 < keep < 0.7 and not torch.equal(b[k], b[k.replace("ew", "bf")])
    full = ew.make_keep_masks(7, 123, 3)
    shard = ew.make_keep_masks(3, 123, 3, row_offset=2, global_rows=7)
    per = 5 * 2 * 8
    assert torch.equal(full["attr/ew_joint"][2 * per:5 * per], shard["attr/ew_joint"])


def _trainer(model_type, tmp_path, D=64, steps=6, A=30, Vq=60):
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV, pretrain_trainer as PTT
    data = DV.synthetic_dataset(40, Vq, 12, A, R=36, D=D, max_len=6, seed=5, enwiki=dict(n_ctx=50, Lc=7))
    ds = {"train": DV.Dataset(split="train", data=data, seed=1, enwiki=True),
          "val": DV.Dataset(split="val", data=data, seed=2, enwiki=True)}
    cfg = PTT.build_parser().parse_args(["--batch_size", "8", "--max_train_iter", str(steps), "--learning_rate", "0.002",
                                         "--model_type", model_type, "--features_on_device", "1", "--input_workers", "0",
                                         "--input_prefetch", "0"])
    cfg.data_cfg = ds["train"].get_config()
    cfg.vocab = {"vocab": ["w%d" % i for i in range(Vq)], "dict": {"w%d" % i: i for i in range(Vq)}}
    cfg.answer_dict, cfg.ws_dict, cfg.enwiki_dict = data["answer_dict"], data["ws_dict"], data["enwiki_dict"]
    cfg.synthetic, cfg.train_dir = 1, str(tmp_path / ("pre_" + model_type))
    return PTT, PTT.Trainer(cfg, ds), data


@pytest.mark.parametrize("model_type", sorted(TYPES))
def test_trainer_loss_falls_and_checkpoint_feeds_the_vqa_trainer(tmp_path, model_type):
    PTT, t, data = _trainer(model_type, tmp_path)
    assert type(t.model).__module__.endswith(model_type) and t.model.engine.heads == TYPES[model_type]
    losses = []
    for _ in range(10):
        step, _, loss, report, _ = t.run_train_step(False)
        losses.append(loss)
    assert sorted(report) == sorted(ER.report_keys(TYPES[model_type])) and np.isfinite(losses).all()
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    assert t.model.mid_result["obj_enwiki/logit"].shape[:2] == (8, 5)
    ckpt = t.save_checkpoint()
    sd = torch.load(ckpt)
    assert "enwiki_map/learn" in sd and "encode_L_enwiki/rnn/gru_cell/gates/kernel/Adam" in sd
    assert ("wordset_ft/fc/weights" in sd) == ("ws" in TYPES[model_type])
    wdir = PTT.export_word_weights(sd, t.model.vocab, data["answer_dict"], str(tmp_path / "word_weights_model-10"))
    # the VQA trainer: --vlmap_word_weight_dir + --pretrained_param_path of this checkpoint, transferred unchanged
    from tests.test_gpu_trainer import _config, _datasets, _features
    from vqa_transfer_externaldata_amd import trainer
    c, Vq, A = _config(tmp_path, "vlmap_answer", pretrained_param_path=ckpt, vlmap_word_weight_dir=wdir,
                       train_dir=str(tmp_path / "vqa"))
    t2 = trainer.Trainer(c, datasets=_datasets(Vq, A), image_features=_features())
    moved = 0
    for n, v in t2.model.variables().items():
        if n.split("/")[0] in ("q_linear_l", "pooled_linear_l", "joint_fc") and n in sd:
            assert torch.equal(v.cpu(), sd[n]), n
            moved += 1
    assert moved >= 6
    t2.run_train_step(False)


def _dp_case():
    rng = np.random.default_rng(31)
    c = dict(n=5, R=36, D=64, H=32, L=6, W=300, Vq=60, n_ws=15, A=40, n_ctx=25, Lc=7)
    heads = TYPES["vlmap_bf_or_wordset_enwiki_withatt_sp"]
    p = ER.init_params(rng, c["Vq"], c["n_ws"], c["A"], W=c["W"], D=c["D"], H=c["H"], heads=heads, n_ctx=c["n_ctx"])
    batch = ER.add_enwiki_fields(rng, PO.make_batch(rng, 5, c["n"], c["R"], c["D"], c["L"], c["Vq"], c["n_ws"], c["A"]),
                                 c["n_ctx"], c["Lc"])
    return c, heads, p, batch


def _dp_steps(eng, PT, batch, lo, hi, reducer, Bg=5):
    shard = {k: torch.from_numpy(np.ascontiguousarray(v[lo:hi])).cuda() for k, v in batch.items()}
    host = {k: v[lo:hi] for k, v in batch.items()}
    shard.update({k: v for k, v in PT.add_length_sort(dict(host)).items() if k.endswith("/sort")})
    gv = eng.global_valid_counts(host) if reducer is not None else None
    first = None
    for it in range(2):
        masks = eng.make_keep_masks(hi - lo, 21, it, row_offset=lo, global_rows=Bg)
        eng.train_step(shard, masks, 2e-3, allreduce=reducer, global_valid=gv)
        if first is None:
            torch.cuda.synchronize()
            first = (eng.grad_flat.cpu().numpy().copy(), eng.fetch_report(reduce=reducer is not None))
    torch.cuda.synchronize()
    return first[0], first[1], eng.train_flat.cpu().numpy().copy()


def _dp_engine():
    from vqa_transfer_externaldata_amd import pretrain as PT
    c, heads, p, batch = _dp_case()
    eng = PT.PretrainEngine(n=c["n"], R=c["R"], D=c["D"], H=c["H"], W=c["W"], A=c["A"], Vq=c["Vq"], n_ws=c["n_ws"],
                            params=p, heads=heads, n_ctx=c["n_ctx"])
    return PT, eng, batch


def _dp_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from vqa_transfer_externaldata_amd import dp
    PT, eng, batch = _dp_engine()
    lo, hi = dp.shard_bounds(5, rank, world)
    g1, rep, params = _dp_steps(eng, PT, batch, lo, hi, dp.BucketedAllReduce())
    if rank == 0:
        np.savez(out_path, g1=g1, params=params, rep_keys=np.array(sorted(rep)), rep=np.array([rep[k] for k in sorted(rep)]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_gloo_rehearsal_equals_one_process(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out_path = str(tmp_path / "rank0.npz")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, out_path)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
        assert pr.exitcode == 0
    got = np.load(out_path)
    PT, eng, batch = _dp_engine()
    g1, rep, params = _dp_steps(eng, PT, batch, 0, 5, None)
    for name, (off, cnt) in eng._tab.items():
        if name.endswith("score/fc/biases"):
            continue
        a, b = got["g1"][off:off + cnt], g1[off:off + cnt]
        sc = max(np.abs(b).max(), 1e-12)
        assert np.abs(a - b).max() <= 5e-5 * sc + 1e-10, (name, np.abs(a - b).max(), sc)
    n = eng.n_train
    assert abs(got["g1"][n] - g1[n]) <= 1e-5 * g1[n]
    assert len(got["rep_keys"]) == 19
    for k, v in zip(got["rep_keys"], got["rep"]):
        assert abs(v - rep[str(k)]) <= 1e-5 * max(1.0, abs(rep[str(k)])), (k, v, rep[str(k)])
    d = np.abs(got["params"] - params)
    assert d.max() <= 5e-4, d.max()
