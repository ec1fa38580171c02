#!/usr/bin/env python3
"""Headline benchmark: VQA train samples/sec of model_vlmap_answer at bs 512 per
GPU (BASELINE.json configs[1]) -- one pass of the hot path (forward, backward,
global-norm clip, Adam) over one synthetic batch per step, inputs resident in HBM.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N > 1: one rank per GPU, RCCL all-reduce of the gradient buckets overlapped with
backward; weak scaling = 512 samples per GPU.  Either the driver launches the ranks
(`python -m torch.distributed.run ... bench.py --gpus N`, WORLD_SIZE set) or a plain
`python bench.py --gpus N` starts them itself: the parent spawns torch.distributed.run
as a CHILD process before it touches the GPU (a process that has initialised the GPU is
never re-exec'ed) and forwards rank 0's JSON line.

Prints ONE JSON line (rank 0): the headline (`metric`, `value` in samples/s, `unit`,
`higher_is_better`, `dtype`, `ms_per_step`) and the `roofline` of the dominant kernel (the
v_linear_v forward GEMM, timed with HIP events on its own stream inside the timed
region) plus what the WHOLE step achieves (`roofline.step`: 356 GFLOP over the step time).
A plain run does nothing else: set-up, warm-up, the K timed steps, the outputs of the last
step when --dump-outputs DIR is given (dump_outputs), the line.

--full adds everything that takes passes of its own, after the timed region (each
--no-* option still drops its part): where the step's time goes
(`roofline.groups`: big GEMMs / recurrence / K = 300 GEMMs / small FCs /
HBM-bound kernels, each with its algorithmic work and fraction of its own peak, measured in a
separate pass after the timed region) and the shader clock under it (`roofline.clock`), the
bf16 x 3 experiment (`experiment_bf16x3`), a `cpu_baseline` (torch-CPU port of the same step on
the host cores, N = 1 only), the extractor throughput `vfeat`, the end-to-end leg `e2e`
(BASELINE configs[2]; with N ranks = configs[3]: every rank extracts its own 256 images, no
collective, and trains on them with the bucketed gradient all-reduce) and the cfg-5 pre-training
step `pretrain` (BASELINE configs[4]: global batch 512, sharded over the N ranks).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense f32-input MFMA peak (= vector peak)
HBM_PEAK_TBS = 8.0             # MI355X_MICROARCH.md: HBM3E spec (a streaming copy reaches about 6.3)
STEP_GFLOP = 356.2             # 0.696 GFLOP per sample x 512 (sum of step_groups()'s mfma groups)

CFG = dict(B=512, R=36, D=2048, H=1024, T=14, W=300, A=3000, Vq=16384, N_img=8192, num_train_answer=2250)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-vfeat", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--no-pretrain", action="store_true")
    ap.add_argument("--no-groups", action="store_true")
    ap.add_argument("--no-bf16x3", action="store_true")
    ap.add_argument("--probe", type=str, default="v_linear_v.fwd_gemm")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the group / clock passes, the bf16x3 experiment, the vfeat, e2e "
                         "and pretrain legs and the CPU baseline (the --no-* options drop single ones)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (see dump_outputs)")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` with no launcher around it: start the N ranks as children of a fresh
    torch.distributed.run process.  Nothing in this parent has touched the GPU (torch is not even imported)."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    r = subprocess.run(cmd, env=env)
    return r.returncode


def synth_params(model_type, cfg, seed):
    """Random-init weights of the architecture: Xavier-uniform FCs, GRU
    gate bias 1.0, embeddings U(-0.01, 0.01)."""
    import torch
    from vqa_transfer_externaldata_amd import fusion as F
    g = torch.Generator().manual_seed(seed)
    shapes = F.variable_shapes(model_type, cfg["Vq"], cfg["W"], cfg["D"], cfg["H"], cfg["A"])
    p = {}
    for n, s in shapes.items():
        if n.endswith("embed_map"):
            p[n] = (torch.rand(s, generator=g) * 0.02 - 0.01)
        elif n.endswith("/weights") or n.endswith("/kernel"):
            lim = (6.0 / (s[0] + s[1])) ** 0.5
            p[n] = (torch.rand(s, generator=g) * 2 - 1) * lim
        elif n.endswith("gates/bias") or n.endswith("LayerNorm/gamma"):
            p[n] = torch.ones(s)
        else:
            p[n] = torch.zeros(s)
    return p


def synth_answer_masks(cfg, g, device):
    import torch
    A = cfg["A"]
    am = {"train": (torch.arange(A, device=device) < cfg["num_train_answer"]).float()}
    is_obj = torch.rand(A, generator=g, device=device) < 0.5
    am["obj"], am["attr"] = is_obj.float(), (~is_obj).float()
    am["exist"] = torch.ones(A, device=device)
    return am


def synth_batches(cfg, g, device, n_batches, B=None, N=None):
    import torch
    B = B or cfg["B"]
    N = N or cfg["N_img"]
    T, A = cfg["T"], cfg["A"]
    # Question tokens: uniform over the vocabulary, every id at most once per batch.  The embedding gradient is scatter-
    # added with float atomics; with one addend per row no summation order exists, so a step -- and the whole run, which
    # Adam would otherwise carry last-bit differences through -- computes the same bits every time.
    assert B * T <= cfg["Vq"] - 3, "too few vocabulary ids for distinct tokens"
    batches = []
    scores = torch.tensor([0.3, 0.6, 0.9, 1.0], device=device)
    for _ in range(n_batches):
        tgt = torch.zeros(B, A, device=device)
        for k in range(3):
            ids = torch.randint(0, A, (B,), generator=g, device=device)
            sc = scores[torch.randint(0, 4, (B,), generator=g, device=device)]
            use = torch.rand(B, generator=g, device=device) < (1.0 if k == 0 else 0.5)
            tgt[torch.arange(B, device=device)[use], ids[use]] = sc[use]
        batches.append({
            "image_idx": torch.randint(0, N, (B,), generator=g, device=device, dtype=torch.int64),
            "q_intseq": torch.randperm(cfg["Vq"] - 3, generator=g, device=device)[:B * T].view(B, T).to(torch.int32),
            "q_intseq_len": torch.full((B,), T, dtype=torch.int32, device=device),
            "answer_target": tgt,
        })
    return batches


def synth_inputs(cfg, seed, device, n_batches=4):
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    N, R, D = cfg["N_img"], cfg["R"], cfg["D"]
    table = torch.randn(N, R, D, generator=g, device=device).relu_()
    nbox = torch.full((N,), R, dtype=torch.int32, device=device)
    am = synth_answer_masks(cfg, g, device)
    return table, nbox, am, synth_batches(cfg, g, device, n_batches)


def cpu_baseline(params, table, nbox, am, batch, cfg, steps=5):
    """Torch-CPU fp32 port of the same train step (oracle/torch_ref.py) on the host
    cores, bounded sample: `steps` timed steps at the full bs-512 shape (about 10 s of CPU work at ~200 samples/s)."""
    import numpy as np
    import torch
    from oracle import torch_ref as TR
    n = 512
    tab = table[:n].cpu().numpy()
    b = {k: v.cpu().numpy() for k, v in batch.items()}
    b["image_idx"] = b["image_idx"] % n
    amc = {k: v.cpu().numpy() for k, v in am.items()}
    pn = {k: v.numpy() for k, v in params.items()}
    stepper = TR.CpuTrainStep(pn, tab, nbox[:n].cpu().numpy(), amc, "vlmap_answer", lr=1e-3)
    rng = np.random.default_rng(0)
    masks = {"att": (rng.random((cfg["B"], cfg["R"], cfg["H"])) < 0.8).astype(np.float32),
             "joint": (rng.random((cfg["B"], 2 * cfg["H"])) < 0.5).astype(np.float32)}
    stepper(b, masks)                                   # warm-up (allocations, thread pool)
    ts = []
    for _ in range(steps):
        t0 = time.time()
        stepper(b, masks)
        ts.append(time.time() - t0)
    dt = sorted(ts)[len(ts) // 2]                       # median step: the host cores are shared with other tenants
    return {"value": cfg["B"] / dt, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "value_mean": cfg["B"] * steps / sum(ts),
            "sample": "%d train steps of model_vlmap_answer at bs %d, median step (torch-CPU fp32 restatement, "
                      "oracle/torch_ref.py; the reference TF1 path cannot run here)" % (steps, cfg["B"])}


# v_linear_v forward GEMM: 128x64 tiles, 8 waves of 32x32 (cfg 20), NN layout, plain epilogue -> 144 x 16 = 2304 workgroups
ROOFLINE_KERNEL = "gemm_f32_kernel<128,64,32,32,1,32,0,true,false,0,false,false,512,false>"
PMC_TRAFFIC_FILES = ("r4_pmc_traffic.json", "r3_pmc_traffic.json", "r2_pmc_traffic.json", "r1_pmc_traffic.json")


def name_of(path):
    return os.path.basename(path)


def pmc_traffic():
    """HBM-side bytes per launch of the roofline kernel.  NOT measured in this run: read from the committed
    rocprofv3 PMC passes (profiles/r*_pmc_traffic.json: separate --pmc FETCH_SIZE and --pmc WRITE_SIZE runs of this
    same bench, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950; Infinity-Cache hits are included
    in the fabric-side counter).  Returns (bytes, source) -- (None, None) when no profile names the kernel."""
    want = ROOFLINE_KERNEL.replace(" ", "")
    for name in PMC_TRAFFIC_FILES:
        path = os.path.join(ROOT, "profiles", name)
        try:
            with open(path) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        for k, v in d.items():
            if k.startswith("_") or "grid=" not in k:
                continue
            name, grid = k.replace(" ", "").split("grid=")      # tools/pmc_summary.py truncates long kernel names
            if grid == "2304" and len(name) > 40 and want.startswith(name.rstrip(">")):
                try:
                    return float(v["hbm_bytes_per_launch"]), "profiles/" + name_of(path)
                except (KeyError, TypeError, ValueError):
                    pass
    return None, None


def _vfeat_setup(device, batch):
    import numpy as np
    import torch
    from vqa_transfer_externaldata_amd import vfeat as VF
    rng = np.random.default_rng(1234)
    params = VF.init_random_params(rng, VF.BLOCKS_R101_FULL)
    model = VF.VfeatResnetModel(params, VF.BLOCKS_R101_FULL, device=device)
    g = torch.Generator(device=device).manual_seed(1)
    img = torch.rand(batch, 448, 448, 3, generator=g, device=device) * 255.0
    ys = torch.sort(torch.rand(batch, 36, 2, generator=g, device=device), dim=-1).values
    xs = torch.sort(torch.rand(batch, 36, 2, generator=g, device=device), dim=-1).values
    box = torch.stack([ys[..., 0], xs[..., 0], ys[..., 1], xs[..., 1]], dim=-1).contiguous()
    return model, {"image": img, "normal_box": box}


NO_BF16X3 = False      # --no-bf16x3: skip the experiment legs


def _dist_max(x, device):
    """max over the ranks of a host float (1 rank: itself)"""
    import torch
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return float(x)
    t = torch.tensor([float(x)], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def _barrier():
    import torch
    import torch.distributed as dist
    torch.cuda.synchronize()
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()
        torch.cuda.synchronize()


def vfeat_bench(device, batch=128, iters=10, warmup=3, world=1):
    """vfeat imgs/sec (second half of BASELINE.json's metric): slim-style ResNet-101 blocks 1-4 on
    synthetic 448x448 images + 1x1 crop_and_resize of 36 boxes -> [36, 2048] per image (BASELINE
    configs[2] extractor; random-init He weights).  Every iteration is timed on its own (device
    synchronised on both sides); the headline is the MEDIAN, min and max are reported beside it."""
    import numpy as np
    import torch
    from vqa_transfer_externaldata_amd import vfeat as VF
    model, b = _vfeat_setup(device, batch)
    for _ in range(warmup):
        v = model.build(b)
    _barrier()       # N ranks: every rank extracts its own shard of the images (no collective on this path)
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        v = model.build(b)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts)
    dt_rank = float(np.median(ts))
    dt = _dist_max(dt_rank, device)          # the slowest rank's median iteration
    fl = VF.conv_flops_per_image(VF.BLOCKS_R101_FULL, 448, 448)
    out = {"imgs_per_sec": world * batch / dt, "imgs_per_sec_best": batch / float(ts.min()),
           "imgs_per_sec_worst": batch / float(ts.max()), "iters": iters, "warmup": warmup,
           "batch": batch, "image": "448x448x3", "net": "resnet_v1_101 blocks1-4 + "
           "1x1 crop_and_resize of 36 boxes", "gflop_per_image": fl / 1e9, "tflops": world * batch * fl / dt / 1e12,
           "frac_f32_mfma_peak": batch * fl / dt / 1e12 / F32_MFMA_PEAK_TFLOPS, "out_shape": list(v.shape)}
    if world > 1:
        out.update(ranks=world, sharding="by image, %d per rank per iteration, no collective" % batch,
                   imgs_per_sec_rank0=batch / dt_rank)
    return out


def e2e_bench(device, params, steps=5, warmup=2, B=256, world=1, rank=0):
    """BASELINE configs[2]: ResNet-101 vfeat extractor + model_vlmap_answer, bs 256, one GPU.  One step =
    256 synthetic 448x448 images with 36 boxes each through the extractor (vqa/vfeat_extractor_tf_record_memft.py:77-147:
    conv stack -> 1x1 ROI crop -> rows of the [N,36,2048] feature table) and then one train step of the fusion
    model on those 256 images' questions reading the freshly written table rows.  Both stages are inside the timed
    region; the table stays in HBM (the reference round-trips it through an HDF5 file between two programs)."""
    import torch
    from vqa_transfer_externaldata_amd import fusion as F
    cfg = dict(CFG, B=B, N_img=B)
    model, vb = _vfeat_setup(device, B)
    from vqa_transfer_externaldata_amd import dp as PAR
    g = torch.Generator(device=device).manual_seed(77)
    am = synth_answer_masks(cfg, g, device)      # (identical on every rank: drawn before the rank-dependent batches)
    g = torch.Generator(device=device).manual_seed(77 + 1000 * rank)
    batches = synth_batches(cfg, g, device, 2, B=B, N=B)
    table = torch.zeros(B, cfg["R"], cfg["D"], device=device)
    nbox = torch.full((B,), cfg["R"], dtype=torch.int32, device=device)
    rows = torch.arange(B, device=device)
    eng = F.FusionEngine(model_type="vlmap_answer", B=B, R=cfg["R"], D=cfg["D"], H=cfg["H"], T=cfg["T"], W=cfg["W"],
                         A=cfg["A"], Vq=cfg["Vq"], N_img=B, params=params, device=device, global_batch=B * world)
    eng.bind_inputs(table=table, nbox_table=nbox, answer_masks=am)
    reducer = PAR.BucketedAllReduce(timing=True) if world > 1 else None

    def step(i):
        v = model.build(vb)                                  # [B,36,2048]: this rank's images, no collective
        table.index_copy_(0, rows, v)                        # the extractor's write into the dense table
        ka, kj = eng.make_keep_masks(seed=5, step=i, row_offset=rank * B, global_rows=B * world)
        eng.train_step(batches[i % 2], ka, kj, 1e-3, allreduce=reducer)

    for i in range(warmup):
        step(i)
    _barrier()
    if reducer is not None:
        reducer.reset_timing()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    _barrier()
    dt = _dist_max((time.perf_counter() - t0) / steps, device)
    loss = eng.report(global_rows=B * world if world > 1 else None)["answer_train_loss"]
    out = {"samples_per_sec": world * B / dt, "ms_per_step": dt * 1e3, "batch": B * world, "steps": steps, "warmup": warmup,
           "workload": "256 images 448x448 per GPU -> resnet_v1_101 b1-4 + 36-box 1x1 ROI crop -> feature-table rows -> "
                       "model_vlmap_answer train step on the same (image, question) pairs (BASELINE configs[2]; "
                       "N ranks = configs[3]: global batch 256 N, bucketed gradient all-reduce)",
           "final_train_loss": loss}
    if reducer is not None:
        import numpy as np
        ex = reducer.exposed_ms()
        out.update(ranks=world, allreduce_exposed_ms_per_step=float(np.mean(ex)) if len(ex) else None)
    return out


def pretrain_flops(B, n, R, D, H, W, A, L, rows_per_step):
    """GEMM FLOPs of one cfg-5 train step (forward + dW + dX, MAC x 2).  rows_per_step = sum over the time steps of the
    live caption rows (the recurrence and the x-projection only run on captions that are still going)."""
    Bn = B * n
    fwd = (2 * 2 * (B * R + Bn) * 6 * H          # spat_v_linear_v / spat_q_linear_v, both categories
           + 2 * 2 * Bn * W * H                  # wordset_ft
           + 2 * rows_per_step * W * 3 * H       # packed x-projection
           + 2 * rows_per_step * H * 3 * H       # recurrence
           + 2 * 2 * Bn * D * H                  # pooled_linear_l (once per category)
           + 2 * 4 * Bn * H * H + 2 * 4 * Bn * H * 2 * H + 2 * 4 * Bn * 2 * H * A)     # q_linear_l, joint_fc, classifier
    att = 2 * 2 * Bn * R * (H + D)               # score + pooling, both categories (vector ALU, not MFMA; forward)
    return 3 * fwd - 2 * 2 * B * R * 6 * H, 3 * att      # spat_v_linear_v needs no dX


def pretrain_bench(device, steps=10, warmup=3, world=1, rank=0):
    """BASELINE configs[4], stage 1: the cfg-5 pre-training step (vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp.py +
    vlmap_memft/trainer.py:129-137) at GLOBAL batch 512 images (x 5 entries x 2 categories, obj3000 + attr1000 answers,
    captions <= 10 tokens); with N ranks the 512 images are sharded over them (strong scaling, as configs[4] says
    'bs=512 on 8 GPUs') and the gradients meet in the bucketed all-reduce overlapped with the backward phases."""
    import numpy as np
    import torch
    from vqa_transfer_externaldata_amd import dataset_vlmap as DV, dp as PAR, pretrain as PT
    Bg, n, R, D, H, L, W, Vq, n_ws, A = 512, 5, 36, 2048, 1024, 10, 300, 5000, 2000, 4000
    rng = np.random.default_rng(0)
    p = PT.init_random_params(rng, Vq, n_ws, A, W=W, D=D, H=H)
    ds = DV.Dataset(split="train", data=DV.synthetic_dataset(Bg, Vq, n_ws, A, R=R, D=D, max_len=L, seed=0), seed=0)
    batch = next(DV.create_ops(Bg, ds, is_train=True, shuffle=False))
    batch = {k: v for k, v in batch.items() if v.dtype.kind in "fi" and k != "image_id"}
    lo, hi = PAR.shard_bounds(Bg, rank, world)
    gv = tuple(float(np.clip(batch[k + "_blank_fill/num"], 0, n).sum()) for k in PT.KINDS)
    shard = {k: v[lo:hi] for k, v in batch.items()}
    B = hi - lo
    sort_info = {k: v for k, v in PT.add_length_sort(dict(shard)).items() if k.endswith("/sort")}
    eng = PT.PretrainEngine(n=n, R=R, D=D, H=H, W=W, A=A, Vq=Vq, n_ws=n_ws, params=p, device=device)
    db = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in shard.items()}
    db.update(sort_info)
    reducer = PAR.BucketedAllReduce(timing=True) if world > 1 else None

    def step(i):
        masks = eng.make_keep_masks(B, 1, i, row_offset=lo, global_rows=Bg)
        eng.train_step(db, masks, 1e-3, allreduce=reducer, global_valid=gv if world > 1 else None)

    for i in range(warmup):
        step(i)
    _barrier()
    if reducer is not None:
        reducer.reset_timing()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    _barrier()
    dt = _dist_max((time.perf_counter() - t0) / steps, device)
    rep = eng.fetch_report(reduce=world > 1)
    # live caption rows of the GLOBAL batch (captions of both categories, lengths clipped to L)
    lens = np.concatenate([np.clip(batch[k + "_blank_fill/blanks_len"].reshape(-1), 0, L) for k in PT.KINDS])
    gemm_fl, att_fl = pretrain_flops(Bg, n, R, D, H, W, A, L, float(lens.sum()))
    out = {"ms_per_step": dt * 1e3, "images_per_sec": Bg / dt, "entries_per_sec": 2 * Bg * n / dt, "global_batch": Bg,
           "steps": steps, "warmup": warmup, "layernorm": "shared" if eng.ln_shared else "per call site",
           "gemm_gflop_per_step": gemm_fl / 1e9, "mfma_floor_ms": gemm_fl / (F32_MFMA_PEAK_TFLOPS * 1e12) * 1e3 / world,
           "tflops": gemm_fl / dt / 1e12, "frac_f32_mfma_peak": gemm_fl / dt / 1e12 / (F32_MFMA_PEAK_TFLOPS * world),
           "total_loss": rep["total_loss"],
           "workload": "cfg-5 pre-training step (vlmap_bf_or_wordset_withatt_sp): fwd + bwd + clip + Adam, global batch 512 "
                       "images x 5 entries x {object, attribute}, 4000 answers, captions of 1..10 tokens encoded as one "
                       "length-sorted batch (BASELINE configs[4], stage 1)"}
    if world == 1 and not NO_BF16X3:
        # the same step with the opt-in bf16 x 3 mode on the big whole-tile products (an EXPERIMENT, see experiment_bf16x3)
        from vqa_transfer_externaldata_amd import _lib
        lib = _lib.load()
        _lib.check(lib.vqa_gemm_bf16x3_set_mode(1), "vqa_gemm_bf16x3_set_mode")
        try:
            for i in range(2):
                step(i)
            torch.cuda.synchronize()
            tb = time.perf_counter()
            for i in range(steps):
                step(2 + i)
            torch.cuda.synchronize()
            out["experiment_bf16x3_ms_per_step"] = (time.perf_counter() - tb) / steps * 1e3
        finally:
            _lib.check(lib.vqa_gemm_bf16x3_set_mode(0), "vqa_gemm_bf16x3_set_mode")
    if reducer is not None:
        ex = reducer.exposed_ms()
        out.update(ranks=world, images_per_rank=B, scaling="strong",
                   allreduce_exposed_ms_per_step=float(np.mean(ex)) if len(ex) else None,
                   allreduce_bytes_per_step=int(eng.grad_flat.numel() * 4))
    return out


# ---- where the step's time goes: launch groups of the fusion step (labels of csrc/probe.hip), their algorithmic work
def step_groups(cfg):
    B, R, D, H, T, W, A, Vq = (cfg[k] for k in ("B", "R", "D", "H", "T", "W", "A", "Vq"))
    Wp = (W + 1 + 3) // 4 * 4
    n_param = Vq * W + D * H + 3 * H + (W + H) * 3 * H + 3 * H + H * H + 3 * H + H + 1      # trainable floats (vlmap_answer)
    f4 = 4.0
    return {
        "big_gemms": {"bound": "mfma", "labels": ["v_linear_v.fwd_gemm", "v_linear_v.dw_gemm", "gru.dwh_gemm"],
                      "work": 2.0 * B * R * D * H * 2 + 2.0 * H * 3 * H * T * B,
                      "what": "v_linear_v forward and weight gradient (K 2048 / M 18432), GRU recurrent weight gradients"},
        "recurrence": {"bound": "mfma", "labels": ["gru.fwd", "gru.bwd"], "work": 2 * 2.0 * B * H * 3 * H * T,
                       "what": "GRU recurrence, forward and back-propagation through time: one weight-stationary persistent launch per direction (csrc/gru_ws.hip; the 28 + 28 fused step kernels where it does not apply)"},
        "k300_gemms": {"bound": "mfma", "labels": ["gru.xp_gemm", "gru.dx_gemm", "gru.dwx_gemm"],
                       "work": 2.0 * T * B * 3 * H * (2 * W + Wp),
                       "what": "packed x-projection of all time steps, its dx and its weight gradient (K or N = 300)"},
        "small_fc": {"bound": "mfma", "labels": ["fc.fwd_gemm", "fc.dw_gemm", "fc.dx_gemm", "head.fwd_gemm", "head.bwd_gemm"],
                     "work": 2.0 * B * (2 * H * H + D * H + 2 * H * H + 2 * H * A)            # forward
                             + 2.0 * B * (2 * H * A + 2 * H * H + D * H + H * H + 2 * H * H),  # dX of the frozen layers, dW + dX of q_linear_v
                     "what": "M = 512 GEMMs: q_linear_v, pooled_linear_l, q_linear_l, joint_fc, answer head"},
        "hbm_kernels": {"bound": "hbm",
                        "labels": ["gather", "v_linear_v.ln_fwd", "v_linear_v.ln_bwd", "fc.ln_fwd", "fc.ln_bwd",
                                   "attn_pool.fwd", "attn_pool.bwd", "embed.fwd", "embed.bwd", "eltwise", "loss.fwd",
                                   "masks", "optimizer"],
                        "work": f4 * (2 * B * R * D                                  # gather: read + write V_ft
                                      + 2 * B * R * H + 3 * B * R * H               # LayerNorm 36x1024 forward / backward
                                      + (B * R * H + B * R * D) + B * R * H / 4      # attention forward: v, V, keep mask (u8)
                                      + (2 * B * R * H + B * R * D) + B * R * H / 4  # attention backward: v, dv, V, mask
                                      + 2 * T * B * Wp + 2 * T * B * W              # embedding lookup / scatter-add
                                      + 3 * B * A + 12 * B * H                      # loss (logit, target, dlogit), small LNs
                                      + 7 * n_param)                                 # clip + Adam: 4 reads + 3 writes
                                + B * R * H + 2 * B * H,                             # mask generation (u8)
                        "what": "gather, LayerNorms, attention + pooling, embedding, loss, dropout masks, clip + Adam"},
    }


def clock_pass(eng, lib, batches, rank, step_ms, steps=12):
    """The shader clock the train step runs at: `steps` extra steps with the library's clock sampler (a few sleeping
    single-wave workgroups on a side stream that count shader cycles per 0.5 ms of real time, csrc/probe.hip) beside them.
    Separate from the timed region.  The f32 MFMA peak of the roofline (157.3 TFLOP/s) is 2.4 GHz x 256 CUs x 256
    flop/cycle; under sustained matrix work the chip holds less, and every fraction below is ALSO given against the peak
    at the measured clock."""
    import numpy as np
    import torch
    from vqa_transfer_externaldata_amd import _lib
    us, wgs = 500.0, 8
    n = max(4, int(steps * step_ms * 1e3 / us))
    out = torch.zeros(wgs, n, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    for i in range(2):
        ka, kj = eng.make_keep_masks(seed=11 + rank, step=2000 + i)
        eng.train_step(batches[i % len(batches)], ka, kj, 1e-3)
    torch.cuda.synchronize()
    # The sampler's waves sit on eight CUs for the whole pass; the weight-stationary recurrence (csrc/gru_ws.hip) needs every
    # SIMD's whole register file on all 256 CUs and would wait for the sampler to leave.  The sampled steps therefore run the
    # per-step recurrence kernels (same matrix work, 56 launches instead of 2 per direction).
    lib.vqa_gru_ws_set_mode(0)
    try:
        _lib.check(lib.vqa_clock_sample(us, n, wgs, C.c_void_p(out.data_ptr()), C.c_void_p(side.cuda_stream)), "vqa_clock_sample")
        for i in range(steps + 2):
            ka, kj = eng.make_keep_masks(seed=11 + rank, step=2002 + i)
            eng.train_step(batches[i % len(batches)], ka, kj, 1e-3)
        torch.cuda.synchronize()
    finally:
        lib.vqa_gru_ws_set_mode(-1)
    g = out.cpu().numpy()[:, 1:-1].ravel()         # (first and last period: ramps)
    sane = g[(g > 0.3) & (g < 4.0)]                # (a period in which the cycle counter restarted reads as 1e10+ GHz: seen once)
    dropped = int(g.size - sane.size)
    g = sane if sane.size else g
    ghz = float(g.mean())                          # equal periods: cycles of the whole pass / its duration
    return {"shader_ghz": ghz, "median": float(np.median(g)), "min": float(g.min()), "max": float(g.max()), "nominal_ghz": 2.4,
            "f32_mfma_peak_at_clock": F32_MFMA_PEAK_TFLOPS * ghz / 2.4,
            "dropped_samples": dropped,
            "how": "mean over %d samples of %.1f ms on %d sampler waves (one per XCD) while %d train steps ran; "
                   "cycles = s_memtime, time = s_memrealtime (100 MHz); the sampled steps run the per-step recurrence kernels (the "
                   "weight-stationary launches cannot share a CU with the sampler's waves)" % (g.size, us / 1e3, wgs, steps)}


def groups_pass(eng, lib, batches, cfg, rank, steps=10):
    """`steps` extra train steps with every launch group probed (HIP events on the step's stream around each group; the
    optimizer and the mask generator, which are separate C calls, through torch events on the same stream).  Run AFTER
    the timed region: the headline number carries one probe only."""
    import numpy as np
    import torch
    from vqa_transfer_externaldata_amd import _lib
    _lib.check(lib.vqa_probe_enable(b"*", 64 * steps), "vqa_probe_enable")
    py = {"masks": [], "optimizer": [], "step": []}

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    for i in range(steps):
        e0 = ev()
        ka, kj = eng.make_keep_masks(seed=7 + rank, step=1000 + i)
        e1 = ev()
        eng.forward(batches[i % len(batches)], ka, kj, want_dz=True)
        eng.backward()
        e2 = ev()
        eng.optimizer_step(1e-3)
        e3 = ev()
        py["masks"].append((e0, e1)); py["optimizer"].append((e2, e3)); py["step"].append((e0, e3))
    torch.cuda.synchronize()
    buf = C.create_string_buffer(4096)
    lib.vqa_probe_labels(buf, 4096)
    per_label = {}
    for lab in buf.value.decode().split("\n"):
        if not lab:
            continue
        ms = (C.c_float * (64 * steps))()
        n = C.c_int()
        _lib.check(lib.vqa_probe_read_label(lab.encode(), ms, 64 * steps, C.byref(n)), "vqa_probe_read_label")
        per_label[lab] = float(np.sum(ms[:n.value])) / steps * 1e3                   # us per step
    lib.vqa_probe_disable()
    for k, pairs in py.items():
        per_label[k] = float(np.mean([a.elapsed_time(b) for a, b in pairs])) * 1e3
    step_us = per_label.pop("step")
    groups, covered = {}, 0.0
    for name, g in step_groups(cfg).items():
        us = sum(per_label.get(l, 0.0) for l in g["labels"])
        covered += us
        if g["bound"] == "mfma":
            ach, peak, unit = g["work"] / (us * 1e-6) / 1e12 if us else None, F32_MFMA_PEAK_TFLOPS, "TFLOP/s"
        else:
            ach, peak, unit = g["work"] / (us * 1e-6) / 1e12 if us else None, HBM_PEAK_TBS, "TB/s"
        groups[name] = {"us_per_step": us, "bound": g["bound"], "work": g["work"], "work_unit": "flop" if g["bound"] == "mfma" else "bytes",
                        "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak if ach else None, "what": g["what"],
                        "labels_us": {l: per_label.get(l, 0.0) for l in g["labels"]}}
    groups["other"] = {"us_per_step": step_us - covered,
                       "what": "launch gaps between groups, memsets, weight packing, report reduction (step - sum of groups)"}
    return groups, step_us


DUMP_SAMPLE = 1 << 20          # elements kept of a larger variable or gradient
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(eng, out_dir):
    """--dump-outputs: what the last timed train step handed its caller, one DIR/<name>.npy each -- `report` (the 13 report
    scalars, float64), `logit` [B, A] and `pred` [B] (float32), and for every trainable variable its value after the Adam
    update (`param.<name>`) and its gradient (`grad.<name>`), float32, '/' of the variable name written as '.'.  A variable
    of more than DUMP_SAMPLE elements is written as a sample of that many flat positions in ascending order, drawn from a
    seed derived from its name: the same positions in every run.  About 46 MB at the benchmark's shape.  With the same
    arguments two runs of one build write the same bits (seeded inputs, distinct tokens per batch: synth_batches)."""
    import zlib
    import numpy as np
    import torch
    eng.check_recurrence()
    B, A = eng.dims.B, eng.dims.A
    arrays = {"report": eng.tensor("report")[:13].cpu().numpy().astype(np.float64),
              "logit": eng.tensor("logit")[:B * A].view(B, A).cpu().numpy(),
              "pred": eng.tensor("pred")[:B].cpu().numpy().astype(np.float32)}
    for name in eng.train_names:
        key = name.replace("/", ".")
        p, g = eng.params[name].reshape(-1), eng.grads[name].reshape(-1)
        if p.numel() > DUMP_SAMPLE:
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            sel = torch.from_numpy(np.sort(rng.choice(p.numel(), DUMP_SAMPLE, replace=False))).to(p.device)
            p, g = p[sel], g[sel]
        arrays["param." + key] = p.cpu().numpy()
        arrays["grad." + key] = g.cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, "dump of %d bytes exceeds %d" % (total, DUMP_MAX_BYTES)
    os.makedirs(out_dir, exist_ok=True)
    for key, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (key, a.dtype)
        np.save(os.path.join(out_dir, key + ".npy"), a)
    return total


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    global NO_BF16X3
    NO_BF16X3 = bool(args.no_bf16x3)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args, argv))

    import numpy as np
    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = None
    ndev = torch.cuda.device_count()       # does not initialise the GPU
    if world > 1:
        import torch.distributed as dist
        backend = os.environ.get("VQA_BENCH_BACKEND", "nccl")      # "gloo" = rehearsal on a 1-GPU box
        if backend == "nccl":
            if ndev < world:
                raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible (set VQA_BENCH_BACKEND=gloo to rehearse "
                                 "several ranks on one GPU)" % (world, ndev))
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    if os.environ.get("VQA_BENCH_DRY_RUN"):
        # rehearsal of the launch path on a box without (enough) GPUs: everything up to the first GPU call -- argument
        # parsing, the self-spawned torch.distributed.run, rendezvous on 127.0.0.1, rank / shard bookkeeping -- then out
        from vqa_transfer_externaldata_amd import dp as PAR
        lo, hi = PAR.shard_bounds(CFG["B"] * world, rank, world)
        mine = torch.tensor([float(hi - lo), float(rank)])
        if world > 1:
            dist.all_reduce(mine)
            dist.barrier()
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "backend": backend, "global_batch": int(mine[0]),
                              "rank_sum": int(mine[1]), "steps": args.steps, "warmup": args.warmup}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    local_rank = local_rank % max(ndev, 1)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    import __graft_entry__ as ge
    if rank == 0 and not os.path.exists(os.path.join(ROOT, "vqa-transfer-externaldata_amd", "libvqahot.so")):
        ge.build()
    if world > 1:
        dist.barrier()
    from vqa_transfer_externaldata_amd import _lib, fusion as F
    from vqa_transfer_externaldata_amd import dp as PAR

    cfg = dict(CFG)
    params = synth_params("vlmap_answer", cfg, seed=1234)
    table, nbox, am, batches = synth_inputs(cfg, seed=1234 + rank, device=device)
    eng = F.FusionEngine(model_type="vlmap_answer", B=cfg["B"], R=cfg["R"], D=cfg["D"], H=cfg["H"], T=cfg["T"],
                         W=cfg["W"], A=cfg["A"], Vq=cfg["Vq"], N_img=cfg["N_img"], params=params, device=device,
                         global_batch=cfg["B"] * world)
    eng.bind_inputs(table=table, nbox_table=nbox, answer_masks=am)
    reducer = PAR.BucketedAllReduce(timing=True) if world > 1 else None
    lib = _lib.load()
    if os.environ.get("VQA_GRU_CFG"):
        _lib.check(lib.vqa_gemm_set_gru_config(int(os.environ["VQA_GRU_CFG"])), "vqa_gemm_set_gru_config")
    if os.environ.get("VQA_GEMM_CFG"):     # tuning only: forces ONE tile config on every plain GEMM
        _lib.check(lib.vqa_gemm_set_config(int(os.environ["VQA_GEMM_CFG"])), "vqa_gemm_set_config")

    def step(i):
        ka, kj = eng.make_keep_masks(seed=99 + rank, step=i)       # fresh dropout masks every step
        eng.train_step(batches[i % len(batches)], ka, kj, 1e-3, allreduce=reducer)

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    if reducer is not None:
        reducer.reset_timing()
    _lib.check(lib.vqa_probe_enable(args.probe.encode(), max(args.steps, 1)), "vqa_probe_enable")
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())

    ms = (C.c_float * max(args.steps, 1))()
    n = C.c_int()
    _lib.check(lib.vqa_probe_read(ms, args.steps, C.byref(n)), "vqa_probe_read")
    lib.vqa_probe_disable()
    loss = eng.report()["answer_train_loss"]
    assert np.isfinite(loss), "training diverged"
    n_grad_floats = eng.grad_flat.numel()
    if args.dump_outputs and rank == 0:
        dump_outputs(eng, args.dump_outputs)

    groups, groups_step_us, clock = (None, None, None)
    if args.full and not args.no_groups:
        groups, groups_step_us = groups_pass(eng, lib, batches, cfg, rank)
        if world == 1:
            clock = clock_pass(eng, lib, batches, rank, dt / args.steps * 1e3)
    # EXPERIMENT leg (never the headline): the same step with the big whole-tile GEMMs on the bf16 matrix pipe through
    # three-way operand splits (csrc/gemm_bf16x3.hip) -- an opt-in numerics mode whose products are f32-equivalent
    bf16x3 = None
    if args.full and not args.no_bf16x3 and world == 1:
        _lib.check(lib.vqa_gemm_bf16x3_set_mode(1), "vqa_gemm_bf16x3_set_mode")
        try:
            for i in range(3):
                step(10000 + i)
            torch.cuda.synchronize()
            tb = time.perf_counter()
            for i in range(args.steps):
                step(10003 + i)
            torch.cuda.synchronize()
            db = time.perf_counter() - tb
        finally:
            _lib.check(lib.vqa_gemm_bf16x3_set_mode(0), "vqa_gemm_bf16x3_set_mode")
        bf16x3 = {"ms_per_step": db / args.steps * 1e3, "samples_per_sec": cfg["B"] * args.steps / db,
                  "speedup_vs_headline": dt / db,
                  "dtype": "f32 operands split into 3 bf16 pieces, 6 v_mfma_f32_32x32x16_bf16 products per f32 product, f32 "
                           "accumulate (f32-equivalent products, not bit-identical sums)",
                  "routed": "whole-tile NN / TN products of >= 2^32 multiply-adds: v_linear_v forward and weight gradient, "
                            "recurrent weight gradients; everything else on the exact f32 MFMA",
                  "peak": "bf16 MFMA 2516 TFLOP/s dense / 6 products = 419 TFLOP/s of f32-equivalent work for the routed GEMMs",
                  "parity": "the full -m gpu suite passes with VQA_HOT_BF16X3=1 at the f32 path's bars (logits 1e-3, argmax "
                            "bit-exact, gradients 5e-4); profiles/r3_bf16x3_suite.txt",
                  "note": "opt-in experiment: VQA_HOT_BF16X3=1 or vqa_gemm_bf16x3_set_mode(1); the headline value above is "
                          "the exact f32 MFMA path"}
    # the other legs run on EVERY rank (each is sharded like its config says); rank 0 prints
    legs = {}
    del eng
    torch.cuda.empty_cache()
    if args.full and not args.no_vfeat:
        legs["vfeat"] = vfeat_bench(device, world=world)
        torch.cuda.empty_cache()
    if args.full and not args.no_e2e:
        legs["e2e"] = e2e_bench(device, params, world=world, rank=rank)
        torch.cuda.empty_cache()
    if args.full and not args.no_pretrain:
        legs["pretrain"] = pretrain_bench(device, world=world, rank=rank)
        torch.cuda.empty_cache()

    if rank == 0:
        # the WORST group that matters: lowest fraction of its own bound among the groups that take >= 5 % of the step, named
        # beside the best big kernel so that `roofline.frac` cannot be read as the step's
        worst = None
        if groups:
            def lowest(bound):
                cand = [(g["frac"], k) for k, g in groups.items() if g.get("frac") is not None and g.get("bound") == bound
                        and g["us_per_step"] >= 0.05 * groups_step_us]
                if not cand:
                    return None
                f_, k_ = min(cand)
                g_ = groups[k_]
                return {"group": k_, "frac": f_, "bound": g_["bound"], "achieved": g_["achieved"], "peak": g_["peak"],
                        "unit": g_["unit"], "us_per_step": g_["us_per_step"], "share_of_step": g_["us_per_step"] / groups_step_us,
                        "what": g_["what"]}
            # same bound as the headline kernel (f32 MFMA): the recurrence; and the HBM-bound kernels against the 8 TB/s spec
            worst = lowest("mfma")
            if worst is not None:
                worst["hbm"] = lowest("hbm")
        kern_ms = float(np.mean(ms[:n.value])) if n.value else float("nan")
        # algorithmic FLOPs of the probed kernel: v_linear_v fwd = 2*B*R*D*H
        flops = 2.0 * cfg["B"] * cfg["R"] * cfg["D"] * cfg["H"]
        achieved = flops / (kern_ms * 1e-3) / 1e12
        traffic, traffic_src = pmc_traffic()
        step_ms = dt / args.steps * 1e3
        step_tflops = STEP_GFLOP * 1e9 / (step_ms * 1e-3) / 1e12
        out = {
            "metric": "VQA train samples/sec (img+question) at bs512",
            "value": cfg["B"] * world * args.steps / dt,
            "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": step_ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "ranks": dist.get_world_size() if world > 1 else 1,
            "backend": (dist.get_backend() if world > 1 else "none"),
            "config": {"workload": "model_vlmap_answer train step (fwd+bwd+clip+Adam), bs 512 per GPU, "
                                   "36x2048 precomputed region features resident in HBM, 14-token questions, "
                                   "3000 answers (BASELINE configs[1])",
                       "global_batch": cfg["B"] * world, "Vq": cfg["Vq"], "table_images": cfg["N_img"],
                       "parallelism": "dp%d" % world if world > 1 else "single"},
            "roofline": {"kernel": ROOFLINE_KERNEL + " (v_linear_v forward GEMM, M=18432 N=1024 K=2048, "
                                   "v_mfma_f32_32x32x2_f32)",
                         "bound": "mfma", "achieved": achieved, "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / F32_MFMA_PEAK_TFLOPS, "traffic": traffic,
                         "traffic_unit": "bytes/launch (L2<->fabric, PMC; algorithmic minimum 235e6)",
                         "traffic_source": ("%s (committed rocprofv3 --pmc passes of this bench, not measured in "
                                            "this run)" % traffic_src) if traffic_src else None,
                         "kernel_ms": kern_ms, "samples": n.value,
                         "clock_note": "kernel_ms is measured live with HIP events on the kernel's stream in an unprofiled "
                                       "run; under rocprofv3 the same kernel runs ~4-5 % longer (profiles/r4_trace_summary.txt: "
                                       "the profiler holds the GPU at a lower sustained clock), so frac recomputed from the "
                                       "committed trace is lower by that ratio",
                         # what the WHOLE step achieves against the same peak, and where its time goes
                         "step": {"flops": STEP_GFLOP * 1e9, "ms": step_ms, "achieved": step_tflops,
                                  "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": step_tflops / F32_MFMA_PEAK_TFLOPS,
                                  "frac_at_clock": (step_tflops / clock["f32_mfma_peak_at_clock"]) if clock else None},
                         "clock": clock,
                         "frac_at_clock": (achieved / clock["f32_mfma_peak_at_clock"]) if clock else None,
                         "worst_group": worst,
                         "groups": groups,
                         "groups_note": ("per-group times from a separate pass of 10 steps with HIP events around every "
                                         "launch group (%.1f us per step in that pass, events included); `frac` of a group "
                                         "is against ITS bound's peak (157.3 TFLOP/s f32 MFMA, 8 TB/s HBM)"
                                         % groups_step_us) if groups else None},
            "final_train_loss": loss,
        }
        if bf16x3 is not None:
            out["experiment_bf16x3"] = bf16x3
        if reducer is not None:
            ex = reducer.exposed_ms()
            out["allreduce_exposed_ms_per_step"] = float(np.mean(ex)) if len(ex) else None
            out["allreduce_bytes_per_step"] = int(n_grad_floats * 4)
        out.update(legs)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(params, table, nbox, am, batches[0], cfg)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
