"""ResNet-101 (blocks 1-4) @448 region-feature extraction throughput; usage: vfeat_bench.py [batch] [iters]
[--precision f32|bf16] [--ab_precision] [--layers] [--distance]

`--ab_precision` builds the extractor twice, f32 and bf16 (same parameters, same batch), and alternates their passes in one
process: 3 warm-up and `iters` timed passes each, median and spread (min .. max) of both and their ratio.
`--layers` times every distinct convolution shape of the trunk after the stem in isolation (HIP events, 5 launches after 2
warm-up ones) in both precisions, with the algorithmic FLOPs and bytes of the shape and the grid the bf16 kernel launches
(to find the layer in a kernel trace).
`--distance` prints how far the bf16 features of one image are from the f32 features.
Without options the output is the one f32 line as before."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.environ.get("VQA_HOT_LIB"):      # another build of the library (same-box A/B of compile-time choices)
    from vqa_transfer_externaldata_amd import _lib as _l0
    _l0._LIB_PATH = os.path.abspath(os.environ["VQA_HOT_LIB"])
from vqa_transfer_externaldata_amd import vfeat as VF  # noqa: E402

_ap = argparse.ArgumentParser()
_ap.add_argument("batch", nargs="?", type=int, default=16)
_ap.add_argument("iters", nargs="?", type=int, default=3)
_ap.add_argument("--precision", default="f32", choices=list(VF.PRECISIONS))
_ap.add_argument("--ab_precision", action="store_true")
_ap.add_argument("--layers", action="store_true")
_ap.add_argument("--distance", action="store_true")
ARGS = _ap.parse_args()
batch, iters = ARGS.batch, ARGS.iters
rng = np.random.default_rng(1234)
if os.environ.get("VQA_GEMM_CFG"):   # tuning only
    from vqa_transfer_externaldata_amd import _lib
    _lib.load().vqa_gemm_set_config(int(os.environ["VQA_GEMM_CFG"]))
if os.environ.get("VQA_CONV_CFG"):   # tuning only: one tile config for every implicit-GEMM convolution
    from vqa_transfer_externaldata_amd import _lib
    _lib.load().vqa_conv_set_config(int(os.environ["VQA_CONV_CFG"]))
if os.environ.get("VQA_CONV_BF16_CFG"):   # tuning only: one tile for every bf16 convolution
    from vqa_transfer_externaldata_amd import _lib
    _lib.load().vqa_conv_bf16_set_config(int(os.environ["VQA_CONV_BF16_CFG"]))
PEAK_F32 = 157.3
fl = VF.conv_flops_per_image(VF.BLOCKS_R101_FULL, 448, 448)


def make_batch(n):
    g = torch.Generator(device="cuda").manual_seed(1)
    img = torch.rand(n, 448, 448, 3, generator=g, device="cuda") * 255.0
    ys = torch.sort(torch.rand(n, 36, 2, generator=g, device="cuda"), dim=-1).values
    xs = torch.sort(torch.rand(n, 36, 2, generator=g, device="cuda"), dim=-1).values
    return {"image": img, "normal_box": torch.stack([ys[..., 0], xs[..., 0], ys[..., 1], xs[..., 1]], -1).contiguous()}


def layer_shapes(n):
    """distinct (name of the first, k, stride, Ci, Co, H, W) of the trunk's convolutions after the stem -> count"""
    shapes = {}
    h = w = 112
    cin = 64
    for name, base, units, stride in VF.BLOCKS_R101_FULL:
        for i, (depth, db, s) in enumerate(VF.block_units(base, units, stride)):
            ho, wo = ((h - 1) // s + 1, (w - 1) // s + 1) if s > 1 else (h, w)
            convs = [("conv1", 1, 1, cin, db, h, w), ("conv2", 3, s, db, db, h, w), ("conv3", 1, 1, db, depth, ho, wo)]
            if depth != cin:
                convs.insert(0, ("shortcut", 1, 1, cin, depth, ho, wo))      # after the subsample
            for c in convs:
                shapes.setdefault(c[1:], ["%s/unit_%d/%s" % (name, i + 1, c[0]), 0])[1] += 1
            h, w, cin = ho, wo, depth
    return shapes


def time_events(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)])) * 1e3      # us


if ARGS.layers:
    print("every distinct convolution of the ResNet-101 trunk after the stem, batch %d, in isolation (normal random inputs, "
          "HIP events, median of 5): measured" % batch)
    print("%-28s %3s %-22s %9s %9s %7s %8s %8s %8s %8s" % ("first layer of the shape", "n", "k s Ci Co HxW", "f32 us", "bf16 us",
                                                           "ratio", "bf16 TF/s", "bf16 GB/s", "GFLOP", "MB bf16"))
    tot = {"f32": 0.0, "bf16": 0.0}
    for (k, s, Ci, Co, H, W), (name, count) in layer_shapes(batch).items():
        p = {"c/weights": rng.standard_normal((k, k, Ci, Co)).astype(np.float32) * np.sqrt(2.0 / (k * k * Ci))}
        for nm, v in (("gamma", 1.0), ("beta", 0.0), ("moving_mean", 0.0), ("moving_variance", 1.0)):
            p["c/BatchNorm/" + nm] = np.full(Co, v, np.float32)
        cb = VF.ConvBN(p, "c", VF.SLIM_BN_EPS, "cuda", bf16=True)
        Ho, Wo = ((H - 1) // s + 1, (W - 1) // s + 1) if s > 1 else (H, W)
        x = torch.randn(batch, H, W, Ci, device="cuda")
        xb = x.to(torch.bfloat16)
        pad = (1, 1) if k == 3 else (0, 0)
        t32 = time_events(lambda: VF.conv2d(x, cb, stride=s, pad=pad, out_hw=(Ho, Wo), relu=True))
        t16 = time_events(lambda: VF.conv2d_bf16(xb, cb, stride=s, pad=pad, out_hw=(Ho, Wo), relu=True))
        M = batch * Ho * Wo
        flops = 2.0 * M * k * k * Ci * Co
        nbytes = 2.0 * (batch * H * W * Ci + k * k * Ci * Co + M * Co)           # x, w, y once each, bf16
        tot["f32"] += count * t32
        tot["bf16"] += count * t16
        print("%-28s %3d %-22s %9.1f %9.1f %7.2f %8.1f %8.0f %8.2f %8.1f" % (
            name, count, "%d %d %d %d %dx%d" % (k, s, Ci, Co, H, W), t32, t16, t32 / t16, flops / t16 / 1e6, nbytes / t16 / 1e3,
            flops / 1e9, nbytes / 1e6))
        del x, xb, cb
    print("sum over the trunk's layers (count x time): f32 %.2f ms, bf16 %.2f ms, ratio %.2f" % (
        tot["f32"] / 1e3, tot["bf16"] / 1e3, tot["f32"] / tot["bf16"]))
    sys.exit(0)

params = VF.init_random_params(rng, VF.BLOCKS_R101_FULL)

if ARGS.distance:
    b1 = make_batch(1)
    f = VF.VfeatResnetModel(params, VF.BLOCKS_R101_FULL, precision="f32")
    h = VF.VfeatResnetModel(params, VF.BLOCKS_R101_FULL, precision="bf16")
    for key in ("enc_I", "V_ft"):
        f.build(b1), h.build(b1)
        a, r = h.outputs[key].double(), f.outputs[key].double()
        print("bf16 against f32 features, one ResNet-101 image at 448, %s %s: max |d| / max |f32| = %.3e, mean |d| / mean |f32| = "
              "%.3e (measured)" % (key, tuple(r.shape), float((a - r).abs().max() / r.abs().max()),
                                   float((a - r).abs().mean() / r.abs().mean())))
    del f, h

if ARGS.ab_precision:
    b = make_batch(batch)
    models = {pr: VF.VfeatResnetModel(params, VF.BLOCKS_R101_FULL, precision=pr) for pr in VF.PRECISIONS}
    for m in models.values():
        for _ in range(3):
            m.build(b)
    times = {pr: [] for pr in models}
    for _ in range(iters):
        for pr, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.build(b)
            torch.cuda.synchronize()
            times[pr].append(time.perf_counter() - t0)
    med = {pr: float(np.median(v)) for pr, v in times.items()}
    for pr, v in times.items():
        print("%s batch %d: median %.2f ms (min %.2f .. max %.2f over %d alternated passes)  %.1f imgs/s  %.1f TFLOP/s "
              "(%.1f%% of f32 MFMA peak)" % (pr, batch, 1e3 * med[pr], 1e3 * min(v), 1e3 * max(v), iters, batch / med[pr],
                                           batch * fl / med[pr] / 1e12, 100 * batch * fl / med[pr] / 1e12 / PEAK_F32))
    print("pass time ratio f32 / bf16 = %.3f" % (med["f32"] / med["bf16"]))
    sys.exit(0)
if ARGS.distance:
    sys.exit(0)

model = VF.VfeatResnetModel(params, VF.BLOCKS_R101_FULL, precision=ARGS.precision)
b = make_batch(batch)
model.build(b)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(iters):
    model.build(b)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / iters
print("batch %d%s: %.1f imgs/s  %.1f TFLOP/s (%.1f%% of f32 MFMA peak)" % (
    batch, "" if ARGS.precision == "f32" else " " + ARGS.precision, batch / dt, batch * fl / dt / 1e12,
    100 * batch * fl / dt / 1e12 / PEAK_F32))
