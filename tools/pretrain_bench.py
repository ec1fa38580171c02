"""Throughput of the cfg-5 pre-training step (BASELINE configs[4], stage 1) at bs 512 on one MI355X.

`--model_type vlmap_bf_or_wordset_enwiki_withatt_sp | vlmap_bf_enwiki_withatt_sp` or one of the "no composition" models
(vlmap_noc_bf_or_wordset_withatt_sp, vlmap_nocarch_..., vlmap_noc_bf_or_enwiki_withatt_sp) or the adapted-memory model
(vlmap_bf_or_wordset_withatt_sp_adapt) times that model instead and
also prints the analytic MFMA FLOPs per step (flops_per_step) and the rate they give.  `--alternate` builds cfg-5 and the
chosen model in one process and times their steps alternately (each warmed up first), so that both rates come from the
same box and clocks.  `--precision bf16` builds the timed engine(s) with PretrainEngine(precision="bf16");
`--ab_precision` builds the chosen model twice, f32 and bf16 (same parameters, same batch), and alternates their steps
the same way: both medians and their ratio.  `--ab_features` builds it twice with precision="bf16": X on the batch's
features rounded to bf16 and widened to f32, Y with features="bf16" on the rounded features themselves (same parameters,
bit-identical steps), alternated; medians of `steps`, `--repeats` times over, and Y counts as slower only when it is behind
X by more than the spread of X's own medians.  `--ab_encoder` is the same protocol for the bf16 sequence encoder: X =
precision="bf16", Y = X + encoder="bf16" on the same parameters and batch; Y counts as FASTER only when it is ahead of X
by more than that spread.  `--encoder bf16` (with `--precision bf16`) builds the timed engine(s) with it (a kernel trace
of Y alone).  Without options the output is the cfg-5 line as before."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("VQA_HOT_LIB"):      # A/B of two builds of the library on one box (tuning only)
    from vqa_transfer_externaldata_amd import _lib as _l0
    _l0._LIB_PATH = os.environ["VQA_HOT_LIB"]
from vqa_transfer_externaldata_amd import pretrain as PT  # noqa: E402

B, n, R, D, H, L, W, Vq, n_ws, A = 512, 5, 36, 2048, 1024, 10, 300, 5000, 2000, 4000
N_CTX, LC = 5000, 7
_ap = argparse.ArgumentParser()
_ap.add_argument("steps", nargs="?", type=int, default=10)
_ap.add_argument("--model_type", default="vlmap_bf_or_wordset_withatt_sp",
                 choices=sorted(PT.MODEL_HEADS) + sorted(PT.NOC_MODEL_HEADS) + sorted(PT.ADAPT_MODEL_HEADS))
_ap.add_argument("--alternate", action="store_true")
_ap.add_argument("--precision", default="f32", choices=list(PT.PRECISIONS))
_ap.add_argument("--ab_precision", action="store_true")
_ap.add_argument("--ab_features", action="store_true")
_ap.add_argument("--encoder", default="f32", choices=list(PT.ENCODER_FORMATS))
_ap.add_argument("--ab_encoder", action="store_true")
_ap.add_argument("--repeats", type=int, default=5, help="--ab_features / --ab_encoder: how many medians of `steps` per engine")
ARGS = _ap.parse_args()


def flops_per_step(heads, batch, noc=False, adapt=False):
    """Analytic MFMA FLOPs of one training step from the shapes (forward + dX + dW of every GEMM the step runs; the
    recurrences and their x-projections over the tokens the batch actually holds, i.e. the live rows of the sorted
    batch): per encoder 3 * 2 * tokens * (W + H) * 3H; pooled_linear_l over 2 B n rows; q_linear_l, joint_fc and the
    classifier over 2 B n rows per head type; wordset_ft over 2 B n rows.  noc: joint_v and joint_l (H x 2H each) and
    classifier_v and classifier_l (2H x A each) in place of joint_fc and the classifier.  adapt: v_adapt over the B R
    region rows, forward and dW only (the features are an input: no dX), and pooled_linear_l with K = H."""
    Bn = B * n
    tok = lambda key: int(sum(np.asarray(batch["%s_blank_fill/%s" % (k, key)]).sum() for k in PT.KINDS))
    f = 3 * 2 * tok("blanks_len") * (W + H) * 3 * H
    if "ew" in heads:
        f += 3 * 2 * tok("enwiki_context_len") * (W + H) * 3 * H
    f += 3 * 2 * (2 * Bn) * (H if adapt else D) * H
    if adapt:
        f += 2 * 2 * (B * R) * D * H
    branches = 2 if noc else 1
    f += 3 * 2 * (2 * Bn * len(heads)) * (H * H + branches * (H * 2 * H + 2 * H * A))
    if "ws" in heads:
        f += 3 * 2 * (2 * Bn) * W * H
    return float(f)


rng = np.random.default_rng(0)
p = PT.init_random_params(rng, Vq, n_ws, A, W=W, D=D, H=H)
from vqa_transfer_externaldata_amd import dataset_vlmap as DV  # noqa: E402
ds = DV.Dataset(split="train", data=DV.synthetic_dataset(B, Vq, n_ws, A, R=R, D=D, max_len=L, seed=0), seed=0)
batch = next(DV.create_ops(B, ds, is_train=True, shuffle=False))
batch = {k: v for k, v in batch.items() if v.dtype.kind in "fi" and k != "image_id"}
sort_info = {} if os.environ.get("SORT", "1") == "0" else {k: v for k, v in PT.add_length_sort(dict(batch)).items() if k.endswith("/sort")}
steps = ARGS.steps


def model_engines(model_type, engine_kws):
    """the engines (one per keyword set, same parameters), host batch and FLOPs per step of a model"""
    if model_type == "vlmap_bf_or_wordset_withatt_sp":
        return ([PT.PretrainEngine(n=n, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=n_ws, params=p, **kw) for kw in engine_kws], batch,
                flops_per_step(PT.CFG5_HEADS, batch))
    noc, adapt = model_type in PT.NOC_MODEL_HEADS, model_type in PT.ADAPT_MODEL_HEADS
    heads = (PT.NOC_MODEL_HEADS if noc else PT.ADAPT_MODEL_HEADS if adapt else PT.MODEL_HEADS)[model_type]
    if "ew" in heads:
        data = DV.synthetic_dataset(B, Vq, n_ws, A, R=R, D=D, max_len=L, seed=0, enwiki=dict(n_ctx=N_CTX, Lc=LC))
        dse = DV.Dataset(split="train", data=data, seed=0, enwiki=True)
        be = next(DV.create_ops(B, dse, is_train=True, shuffle=False))
        be = {k: v for k, v in be.items() if v.dtype.kind in "fi" and k != "image_id"}
    else:
        be = batch                 # the noc word-set model and the adapt model read cfg-5's batch
    n_ctx = N_CTX if "ew" in heads else None
    pe = PT.init_random_params(rng, Vq, n_ws, A, W=W, D=D, H=H, heads=heads, n_ctx=n_ctx, noc=noc, adapt=adapt)
    engines = [PT.PretrainEngine(n=n, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=n_ws, params=pe, heads=heads, n_ctx=n_ctx,
                                 noc=noc, adapt=adapt, **kw) for kw in engine_kws]
    return engines, be, flops_per_step(heads, be, noc, adapt)


def other_model(model_type, precisions):
    """the engines (one per precision, same parameters), device batch and FLOPs per step of a model other than cfg-5"""
    engines, be, fl = model_engines(model_type, [dict(precision=pr, encoder=ARGS.encoder if pr == "bf16" else "f32") for pr in precisions])
    dbe = {k: torch.from_numpy(v).cuda() for k, v in be.items()}
    if os.environ.get("SORT", "1") != "0":
        dbe.update({k: v for k, v in PT.add_length_sort(dict(be)).items() if k.endswith("/sort")})
    for ee in engines:
        for i in range(3):
            ee.train_step(dbe, ee.make_keep_masks(B, 1, i), 1e-3)
    return engines, dbe, fl


def ab_medians(runs):
    """runs: ((label, engine, device batch), ...), warmed up.  `--repeats` times: `steps` alternated steps, one median
    per engine.  Returns {label: [medians in ms]}."""
    meds = {k: [] for k, _, _ in runs}
    for r in range(ARGS.repeats):
        times = {k: [] for k, _, _ in runs}
        for i in range(steps):
            for k, e, d in runs:
                masks = e.make_keep_masks(B, 1, 3 + r * steps + i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.train_step(d, masks, 1e-3)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        for k in times:
            meds[k].append(1e3 * float(np.median(times[k])))
        print("%s repeat %d: " % (ARGS.model_type, r) + "  ".join("%s %.3f ms" % (k, meds[k][-1]) for k in meds)
              + "  (medians of %d alternated steps)" % steps)
    return meds


if ARGS.ab_encoder:
    (ex, ey), be, fl = model_engines(ARGS.model_type, [dict(precision="bf16"), dict(precision="bf16", encoder="bf16")])
    dbx = {k: torch.from_numpy(v).cuda() for k, v in be.items()}
    if os.environ.get("SORT", "1") != "0":
        dbx.update({k: v for k, v in PT.add_length_sort(dict(be)).items() if k.endswith("/sort")})
    runs = (("X f32 encoder", ex, dbx), ("Y bf16 encoder", ey, dbx))
    for _, e, d in runs:
        for i in range(3):
            e.train_step(d, e.make_keep_masks(B, 1, i), 1e-3)
    meds = ab_medians(runs)
    mx, my = float(np.median(meds["X f32 encoder"])), float(np.median(meds["Y bf16 encoder"]))
    spread = max(meds["X f32 encoder"]) - min(meds["X f32 encoder"])
    verdict = "FASTER" if mx - my > spread else "SLOWER" if my - mx > spread else "no measurable difference"
    print("%s: X %.3f ms, Y %.3f ms (medians of the %d medians), X - Y = %+.3f ms, spread of X's medians %.3f ms -> Y: %s; "
          "flops_per_step %.3f TFLOP; total_loss %.3f / %.3f"
          % (ARGS.model_type, mx, my, ARGS.repeats, mx - my, spread, verdict, fl / 1e12, ex.fetch_report()["total_loss"],
             ey.fetch_report()["total_loss"]))
    sys.exit(0)


if ARGS.ab_features:
    (ex, ey), be, fl = model_engines(ARGS.model_type, [dict(precision="bf16"), dict(precision="bf16", features="bf16")])
    dbx = {k: torch.from_numpy(v).cuda() for k, v in be.items()}
    if os.environ.get("SORT", "1") != "0":
        dbx.update({k: v for k, v in PT.add_length_sort(dict(be)).items() if k.endswith("/sort")})
    t16 = dbx["image_ft"].to(torch.bfloat16).contiguous()
    dbx["image_ft"] = t16.float()
    runs = (("X f32 features", ex, dbx), ("Y bf16 features", ey, dict(dbx, image_ft=t16)))
    # (the timed engines run without deterministic=True, so only their forwards are compared here; the step-level
    # comparison is tests/test_gpu_pretrain_bf16_features.py)
    fwd = []
    for _, e, d in runs:
        e.forward(d, e.make_keep_masks(B, 1, 0))
        fwd.append([e.tensor(k + "/" + t).clone() for k in PT.KINDS for t in ("att", "pooled")] + [e.tensor("report").clone()])
    print("forward of X and Y at these dims (att, pooled, report of both categories): %s"
          % ("bit for bit equal" if all(torch.equal(a, b) for a, b in zip(*fwd)) else "DIFFERENT"))
    for _, e, d in runs:
        for i in range(3):
            e.train_step(d, e.make_keep_masks(B, 1, i), 1e-3)
    meds = ab_medians(runs)
    mx, my = float(np.median(meds["X f32 features"])), float(np.median(meds["Y bf16 features"]))
    spread = max(meds["X f32 features"]) - min(meds["X f32 features"])
    print("%s: X %.3f ms, Y %.3f ms (medians of the %d medians), Y - X = %+.3f ms, spread of X's medians %.3f ms -> Y is %s; "
          "flops_per_step %.3f TFLOP; total_loss %.3f / %.3f"
          % (ARGS.model_type, mx, my, ARGS.repeats, my - mx, spread, "SLOWER" if my - mx > spread else "not slower", fl / 1e12,
             ex.fetch_report()["total_loss"], ey.fetch_report()["total_loss"]))
    print("resident features: N * %d * %d * 2 bytes (bf16) against N * %d * %d * 4 (f32): %.1f against %.1f GB per 100 k images"
          % (R, D, R, D, 1e5 * R * D * 2 / 1e9, 1e5 * R * D * 4 / 1e9))
    sys.exit(0)


if ARGS.ab_precision:
    if ARGS.model_type == "vlmap_bf_or_wordset_withatt_sp":
        engines = [PT.PretrainEngine(n=n, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=n_ws, params=p, precision=pr) for pr in PT.PRECISIONS]
        dba = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        dba.update(sort_info)
        for e in engines:
            for i in range(3):
                e.train_step(dba, e.make_keep_masks(B, 1, i), 1e-3)
        fl = flops_per_step(PT.CFG5_HEADS, batch)
    else:
        engines, dba, fl = other_model(ARGS.model_type, PT.PRECISIONS)
    times = {e.precision: [] for e in engines}
    for i in range(steps):
        for e in engines:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.train_step(dba, e.make_keep_masks(B, 1, 3 + i), 1e-3)
            torch.cuda.synchronize()
            times[e.precision].append(time.perf_counter() - t0)
    med = {k: 1e3 * float(np.median(v)) for k, v in times.items()}
    for e in engines:
        print("%s %s: step %.2f ms (median of %d alternated)  flops_per_step %.3f TFLOP  -> %.1f TFLOP/s; total_loss %.3f"
              % (ARGS.model_type, e.precision, med[e.precision], steps, fl / 1e12, fl / med[e.precision] / 1e9,
                 e.fetch_report()["total_loss"]))
    print("step time ratio f32 / bf16 = %.3f" % (med["f32"] / med["bf16"]))
    sys.exit(0)

eng = PT.PretrainEngine(n=n, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=n_ws, params=p, precision=ARGS.precision, encoder=ARGS.encoder)
db = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
db.update(sort_info)
if any(os.environ.get(k) for k in ("VQA_LN_FAST", "VQA_GRU_CFG", "VQA_ATTN_FAST", "VQA_SOFTMAX_FAST")):   # A/B switches
    from vqa_transfer_externaldata_amd import _lib
    _l = _lib.load()
    if os.environ.get("VQA_LN_FAST"):
        _l.vqa_ln_set_fast(int(os.environ["VQA_LN_FAST"]))
    if os.environ.get("VQA_GRU_CFG"):
        _lib.check(_l.vqa_gemm_set_gru_config(int(os.environ["VQA_GRU_CFG"])), "gru cfg")
    if os.environ.get("VQA_ATTN_FAST"):
        _l.vqa_attn_set_fast(int(os.environ["VQA_ATTN_FAST"]))
    if os.environ.get("VQA_SOFTMAX_FAST"):
        _l.vqa_softmax_set_fast(int(os.environ["VQA_SOFTMAX_FAST"]))
CFG5_TIMED = ARGS.model_type == "vlmap_bf_or_wordset_withatt_sp" or ARGS.alternate
for i in range(3):
    eng.train_step(db, eng.make_keep_masks(B, int(os.environ.get("MASK_SEED", "1")), i), 1e-3)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(steps if CFG5_TIMED else 0):
    eng.train_step(db, eng.make_keep_masks(B, int(os.environ.get("MASK_SEED", "1")), 3 + i), 1e-3)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / max(steps, 1)
rep = eng.fetch_report()
if CFG5_TIMED:
    print("pretrain step %.2f ms  -> %.0f images/s (%.0f blank-fill entries/s); total_loss %.3f"
          % (dt * 1e3, B / dt, 2 * B * n / dt, rep["total_loss"]))

if ARGS.model_type != "vlmap_bf_or_wordset_withatt_sp" or ARGS.alternate:
    NOC, ADAPT = ARGS.model_type in PT.NOC_MODEL_HEADS, ARGS.model_type in PT.ADAPT_MODEL_HEADS
    heads = (PT.NOC_MODEL_HEADS if NOC else PT.ADAPT_MODEL_HEADS if ADAPT else PT.MODEL_HEADS)[ARGS.model_type]
    f5 = flops_per_step(PT.CFG5_HEADS, batch)
    runs = {"vlmap_bf_or_wordset_withatt_sp": (eng, db, f5)}
    if "ew" in heads or NOC or ADAPT:
        (ee,), dbe, fe = other_model(ARGS.model_type, (ARGS.precision,))
        runs[ARGS.model_type] = (ee, dbe, fe)
    order = list(runs) if ARGS.alternate else [ARGS.model_type]
    times = {k: [] for k in order}
    for i in range(steps):
        for k in order:
            e, d, _ = runs[k]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.train_step(d, e.make_keep_masks(B, 1, 3 + steps + i), 1e-3)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    for k in order:
        e, d, f = runs[k]
        ms = 1e3 * float(np.median(times[k]))
        print("%s: step %.2f ms (median of %d)  flops_per_step %.3f TFLOP  -> %.1f TFLOP/s; total_loss %.3f"
              % (k, ms, steps, f / 1e12, f / ms / 1e9, e.fetch_report()["total_loss"]))
    if ARGS.alternate and len(order) == 2:
        r = [runs[k][2] / np.median(times[k]) for k in order]
        print("flop-rate ratio %s / cfg-5 = %.3f" % (order[1], r[1] / r[0]))
