"""Seeded dropout (FusionEngine.train_step(dropout=(seed, step)): the keep bits computed inside the kernels that consume
them) against the explicit masks (make_keep_masks -> vqa_dropout_mask -> uint8 buffers), alternated in ONE process:

  (1) two bs-512 vlmap_answer engines at full dims, X explicit and Y seeded, alternated step by step: the median of
      --iters steps, repeated --repeats times (the spread of X's own medians is the yardstick of the difference), in f32 and
      in precision="bf16", features="bf16".  X's step includes its two mask launches, as a training step does.
  (2) the five entry points that consume a mask, explicit | seeded, at the step's shapes (the explicit side reads a mask
      that already exists; the mask launches are timed on their own)
  (3) the bytes of mask buffers each engine holds

usage: dropout_ab.py [--iters 20] [--repeats 5] [--explicit-only] [--skip-kernels] [--pretrain [--model_type M]]
--explicit-only: leg (1) with X alone (runs on a tree without the seeded mode: the baseline of the explicit step there).
--pretrain: the same legs (1) and (3) for the pre-training step instead (PretrainEngine.train_step(dropout=(seed, step)),
  cfg-5 at bs 512 by default, any of the six model types with --model_type): X's step includes its make_keep_masks
  launches (6 to 14 per step), as a training step does; captions in length order, as the trainer feeds them."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vqa_transfer_externaldata_amd import ops  # noqa: E402

MASK_ATTRS = ("_keep_att", "_keep_joint", "_keep_joint2", "_keep_tile", "_keep_word")


def alternate_us(fs, iters, warmup=3):
    """median (and best) time of every callable, one iteration of each in turn"""
    for _ in range(warmup):
        for f in fs:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fs]
    for _ in range(iters):
        for k, f in enumerate(fs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    return [(sorted(t)[len(t) // 2], min(t)) for t in ts]


def mask_bytes(eng):
    return sum(getattr(eng, a).numel() for a in MASK_ATTRS if hasattr(eng, a))


def bench_step(iters, repeats, explicit_only, mode):
    import bench as BENCH
    from vqa_transfer_externaldata_amd import fusion as F
    cfg = dict(BENCH.CFG)
    dev = torch.device("cuda", 0)
    params = BENCH.synth_params("vlmap_answer", cfg, seed=1234)
    table, nbox, am, batches = BENCH.synth_inputs(cfg, seed=1234, device=dev)
    kw = {}
    if mode == "bf16":
        kw = dict(precision="bf16", features="bf16")
        table = table.to(torch.bfloat16)
    names = ("X",) if explicit_only else ("X", "Y")
    engs = {}
    for name in names:
        e = F.FusionEngine(model_type="vlmap_answer", B=cfg["B"], R=cfg["R"], D=cfg["D"], H=cfg["H"], T=cfg["T"], W=cfg["W"],
                           A=cfg["A"], Vq=cfg["Vq"], N_img=cfg["N_img"], params=params, device=dev, **kw)
        e.bind_inputs(table=table, nbox_table=nbox, answer_masks=am)
        engs[name] = e
    count = {n: 0 for n in names}

    def step(name):
        e, i = engs[name], count[name]
        if name == "X":
            ka, kj = e.make_keep_masks(seed=99, step=i)
            e.train_step(batches[i % len(batches)], ka, kj, 1e-3)
        else:
            e.train_step(batches[i % len(batches)], lr=1e-3, dropout=(99, i))
        count[name] += 1

    print("== (1) train step, vlmap_answer bs %d, %s: X = explicit masks (two mask launches per step), Y = seeded"
          % (cfg["B"], "f32" if mode == "f32" else 'precision="bf16", features="bf16"'), flush=True)
    meds = {n: [] for n in names}
    for r in range(repeats):
        res = alternate_us([lambda n=n: step(n) for n in names], iters)
        for n, (med, best) in zip(names, res):
            meds[n].append(med)
        print("repeat %d: " % r + "   ".join("%s median %.3f ms (best %.3f)" % (n, med / 1e3, best / 1e3)
                                              for n, (med, best) in zip(names, res))
              + ("" if explicit_only else "   X / Y %.4f" % (res[0][0] / res[1][0])), flush=True)
    mid = {n: sorted(meds[n])[repeats // 2] for n in names}
    spread = {n: max(meds[n]) - min(meds[n]) for n in names}
    if explicit_only:
        print("median of the %d medians: X %.3f ms; spread (max - min) of X's medians %.1f us"
              % (repeats, mid["X"] / 1e3, spread["X"]), flush=True)
    else:
        print("median of the %d medians: X %.3f ms, Y %.3f ms, X - Y = %.1f us; spread (max - min) of X's medians %.1f us, of Y's %.1f us"
              % (repeats, mid["X"] / 1e3, mid["Y"] / 1e3, mid["X"] - mid["Y"], spread["X"], spread["Y"]))
        d = mid["X"] - mid["Y"]
        print("verdict: seeded is %s" % ("FASTER than explicit by more than X's own spread" if d > spread["X"] else
                                         "SLOWER than explicit by more than X's own spread" if -d > spread["X"] else
                                         "within X's own spread of explicit"), flush=True)
    print("== (3) mask buffers held: " + ", ".join("%s %.2f MB" % (n, mask_bytes(engs[n]) / 1e6) for n in names), flush=True)
    del engs
    torch.cuda.empty_cache()


PT_DIMS = dict(B=512, n=5, R=36, D=2048, H=1024, L=10, W=300, Vq=5000, n_ws=2000, A=4000)
PT_CTX = dict(n_ctx=5000, Lc=7)


def u8_bytes(obj, seen=None):
    """bytes of the uint8 tensors reachable from obj (dicts, lists, tuples)"""
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return 0
    seen.add(id(obj))
    if torch.is_tensor(obj):
        return obj.numel() if obj.dtype == torch.uint8 else 0
    if isinstance(obj, dict):
        return sum(u8_bytes(v, seen) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(u8_bytes(v, seen) for v in obj)
    return 0


def bench_pretrain(iters, repeats, explicit_only, model_type):
    import numpy as np
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV, pretrain as PT
    d = PT_DIMS
    B = d["B"]
    noc, adapt = model_type in PT.NOC_MODEL_HEADS, model_type in PT.ADAPT_MODEL_HEADS
    heads = (PT.NOC_MODEL_HEADS if noc else PT.ADAPT_MODEL_HEADS if adapt else PT.MODEL_HEADS)[model_type]
    ew = "ew" in heads
    rng = np.random.default_rng(0)
    params = PT.init_random_params(rng, d["Vq"], d["n_ws"], d["A"], W=d["W"], D=d["D"], H=d["H"], heads=heads,
                                   n_ctx=PT_CTX["n_ctx"] if ew else None, noc=noc, adapt=adapt)
    data = DV.synthetic_dataset(B, d["Vq"], d["n_ws"], d["A"], R=d["R"], D=d["D"], max_len=d["L"], seed=0,
                                **({"enwiki": dict(PT_CTX)} if ew else {}))
    ds = DV.Dataset(split="train", data=data, seed=0, enwiki=True if ew else None)
    batch = next(DV.create_ops(B, ds, is_train=True, shuffle=False))
    batch = {k: v for k, v in batch.items() if v.dtype.kind in "fi" and k != "image_id"}
    names = ("X",) if explicit_only else ("X", "Y")
    engs, dbs = {}, {}
    for name in names:
        engs[name] = PT.PretrainEngine(n=d["n"], R=d["R"], D=d["D"], H=d["H"], W=d["W"], A=d["A"], Vq=d["Vq"], n_ws=d["n_ws"],
                                       params=params, heads=heads, n_ctx=PT_CTX["n_ctx"] if ew else None, noc=noc, adapt=adapt)
        dbs[name] = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        dbs[name].update({k: v for k, v in PT.add_length_sort(dict(batch)).items() if k.endswith("/sort")})
    count = {n: 0 for n in names}
    if not explicit_only:       # same results at the timed size: the forward (no atomics in it) of X and Y, bit for bit
        engs["X"].forward(dbs["X"], engs["X"].make_keep_masks(B, 99, 0), want_dz=False)
        engs["Y"].forward(dbs["Y"], None, want_dz=False, dropout=(99, 0))
        torch.cuda.synchronize()
        tape = lambda e: [e.tensor(k + "/" + t) for k in PT.KINDS for t in ("att", "pooled")] + [e.tensor("report")]
        same = all(torch.equal(x, y) for x, y in zip(tape(engs["X"]), tape(engs["Y"])))
        print("forward of X and Y at these dims (att, pooled, report of both categories): %s"
              % ("bit for bit equal" if same else "DIFFERENT"), flush=True)
        if not same:
            raise SystemExit("the seeded forward is not the explicit forward: no time taken")

    def step(name):
        e, i = engs[name], count[name]
        if name == "X":
            e.train_step(dbs[name], e.make_keep_masks(B, 99, i), 1e-3)
        else:
            e.train_step(dbs[name], None, 1e-3, dropout=(99, i))
        count[name] += 1

    print("== (1) pre-training train step, %s bs %d, f32: X = explicit masks (%d mask launches per step), Y = seeded"
          % (model_type, B, len(engs["X"].keep_offsets(B, 0))), flush=True)
    meds = {n: [] for n in names}
    for r in range(repeats):
        res = alternate_us([lambda n=n: step(n) for n in names], iters)
        for n, (med, best) in zip(names, res):
            meds[n].append(med)
        print("repeat %d: " % r + "   ".join("%s median %.3f ms (best %.3f)" % (n, med / 1e3, best / 1e3)
                                              for n, (med, best) in zip(names, res))
              + ("" if explicit_only else "   X / Y %.4f" % (res[0][0] / res[1][0])), flush=True)
    mid = {n: sorted(meds[n])[repeats // 2] for n in names}
    spread = {n: max(meds[n]) - min(meds[n]) for n in names}
    if explicit_only:
        print("median of the %d medians: X %.3f ms; spread (max - min) of X's medians %.1f us"
              % (repeats, mid["X"] / 1e3, spread["X"]), flush=True)
    else:
        print("median of the %d medians: X %.3f ms, Y %.3f ms, X - Y = %.1f us; spread (max - min) of X's medians %.1f us, of Y's %.1f us"
              % (repeats, mid["X"] / 1e3, mid["Y"] / 1e3, mid["X"] - mid["Y"], spread["X"], spread["Y"]))
        dlt = mid["X"] - mid["Y"]
        print("verdict: seeded is %s" % ("FASTER than explicit by more than X's own spread" if dlt > spread["X"] else
                                         "SLOWER than explicit by more than X's own spread" if -dlt > spread["X"] else
                                         "within X's own spread of explicit"), flush=True)
    print("== (3) mask buffers held: " + ", ".join(
        "%s %.2f MB" % (n, sum(u8_bytes(v) for k, v in vars(engs[n]).items() if k != "workspace") / 1e6) for n in names), flush=True)


def bench_kernels(iters):
    import bench as BENCH
    cfg = dict(BENCH.CFG)
    dev = torch.device("cuda", 0)
    B, Rg, D, H = cfg["B"], cfg["R"], cfg["D"], cfg["H"]
    g = torch.Generator(device=dev).manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    print("== (2) kernels at the step's shapes, explicit mask | seeded, alternated, median us (best us)")

    def line(name, fs):
        (mx, bx), (my, by) = alternate_us(fs, iters)
        print("%-44s explicit %8.1f (%8.1f) | seeded %8.1f (%8.1f) | explicit / seeded = %.3fx" % (name, mx, bx, my, by, mx / my),
              flush=True)

    v, qv, w, bias, dp = rn(B, Rg, H), rn(B, H), rn(H) / H ** 0.5, torch.zeros(1, device=dev), rn(B, D)
    nb = torch.full((B,), Rg, dtype=torch.int32, device=dev)
    V32 = torch.relu(rn(B, Rg, D))
    keep = ops.dropout_mask(B * Rg * H, 99, 0, 0.8, dev)
    sd = (99, 0)
    for tag, V, fwd, bwd in (("f32 memory", V32, ops.attn_pool_fwd, ops.attn_pool_bwd),
                             ("bf16 memory", V32.to(torch.bfloat16), ops.attn_pool_fwd_v16, ops.attn_pool_bwd_v16)):
        att, _ = fwd(v, qv, V, nb, w, bias, keep, 0.8)
        assert torch.equal(att, fwd(v, qv, V, nb, w, bias, keep_seed=sd, keep_prob=0.8)[0])
        line("attn_pool_fwd, %s" % tag, [lambda: fwd(v, qv, V, nb, w, bias, keep, 0.8),
                                         lambda: fwd(v, qv, V, nb, w, bias, keep_seed=sd, keep_prob=0.8)])
        line("attn_pool_bwd (+ 2 colsums), %s" % tag, [lambda: bwd(dp, v, qv, V, att, w, keep, 0.8),
                                                       lambda: bwd(dp, v, qv, V, att, w, keep_seed=sd, keep_prob=0.8)])
    del V32
    pre, ds = rn(B, Rg, H), rn(B, Rg)
    gamma, beta = torch.ones(H, device=dev), torch.zeros(H, device=dev)
    _, mean, rstd = ops.ln_relu_fwd(pre.view(B * Rg, H), gamma, beta, rows=Rg)
    line("ln_relu_att_bwd [512,36,1024]", [lambda: ops.ln_relu_att_bwd(ds, qv, w, pre, mean, rstd, gamma, beta, keep, 0.8),
                                           lambda: ops.ln_relu_att_bwd(ds, qv, w, pre, mean, rstd, gamma, beta, keep_seed=sd,
                                                                       keep_prob=0.8)])
    N = 2 * H
    pj, dj = rn(B, N), rn(B, N)
    gj, bj = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    kj = ops.dropout_mask(B * N, 99, 4 * B * Rg * H, 0.5, dev)
    sj = (99, 4 * B * Rg * H)
    _, mj, rj = ops.ln_relu_fwd(pj, gj, bj)
    line("ln_act_fwd joint [512,2048]", [lambda: ops.ln_act_fwd(pj, gj, bj, keepmask=kj, keep_prob=0.5),
                                         lambda: ops.ln_act_fwd(pj, gj, bj, keep_seed=sj, keep_prob=0.5)])
    line("ln_act_bwd joint [512,2048] (+ colsum3)", [lambda: ops.ln_act_bwd(dj, pj, mj, rj, gj, bj, keepmask=kj, keep_prob=0.5),
                                                     lambda: ops.ln_act_bwd(dj, pj, mj, rj, gj, bj, keep_seed=sj, keep_prob=0.5)])
    (ma, ba), (mj_, bj_) = alternate_us([lambda: ops.dropout_mask(B * Rg * H, 99, 0, 0.8, dev),
                                         lambda: ops.dropout_mask(B * N, 99, 0, 0.5, dev)], iters)
    print("the explicit step's mask launches: keep_att [512,36,1024] %.1f (%.1f) us, keep_joint [512,2048] %.1f (%.1f) us"
          % (ma, ba, mj_, bj_))
    print("(every op call allocates its outputs inside the timed region, the same on both sides)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--explicit-only", action="store_true", help="leg (1) with the explicit engine alone")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--modes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--pretrain", action="store_true", help="the pre-training step (PretrainEngine) instead of the VQA step")
    ap.add_argument("--model_type", default="vlmap_bf_or_wordset_withatt_sp", help="with --pretrain: one of the six model types")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dropout_ab.py needs a GPU: a time taken elsewhere says nothing")
    if args.pretrain:
        bench_pretrain(args.iters, args.repeats, args.explicit_only, args.model_type)
        return
    for mode in args.modes:
        bench_step(args.iters, args.repeats, args.explicit_only, mode)
    if not (args.explicit_only or args.skip_kernels):
        bench_kernels(args.iters)


if __name__ == "__main__":
    main()
