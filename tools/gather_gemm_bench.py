"""v_linear_v forward: separate gather + GEMM against the gather fused into the GEMM's operand load
(vqa_gemm_f32_gather), at the bench shape (B 512, R 36, D 2048, H 1024).

Two tables: the bench's (8192 images, 2.4 GB: every row comes from HBM) and one small enough to stay in the Infinity
Cache (256 images, 75 MB, read once before every timed run), which separates what the fused kernel's loop costs from
what the latency of a cold operand costs.  The fused kernel runs in both of its forms: 32-bit offsets into a table below
4 GiB (the default there) and per-lane 64-bit pointers (vqa_gemm_set_gather_ptr: the form of larger tables).

usage: gather_gemm_bench.py [--runs 20] [--calls 10] [--old-lib /path/to/an/older/libvqahot.so]
--old-lib adds that build's vqa_gemm_f32_gather as "old fused".  Every variant is timed `runs` times, round-robin, each
run `calls` back-to-back calls between two events; prints every run and the median."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqa_transfer_externaldata_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--old-lib", default=None)
args = ap.parse_args()

lib = _lib.load()
old = None
if args.old_lib:
    old = C.CDLL(os.path.abspath(args.old_lib))
    old.vqa_gemm_f32_gather.restype, old.vqa_gemm_f32_gather.argtypes = _lib.SIGNATURES["vqa_gemm_f32_gather"]

B, R, D, H = 512, 36, 2048, 1024
P = lambda t: C.c_void_p(t.data_ptr())
g = torch.Generator(device="cuda").manual_seed(0)
W = torch.randn(D, H, device="cuda", generator=g) * 0.02
bias = torch.zeros(H, device="cuda")
V = torch.empty(B * R, D, device="cuda"); nb = torch.empty(B, dtype=torch.int32, device="cuda")
out = torch.empty(B * R, H, device="cuda"); out2 = torch.empty_like(out); V2 = torch.empty_like(V)


def timed(f, calls):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def bench_table(N, label, touch):
    table = torch.randn(N, R, D, device="cuda", generator=g).relu_()
    nbox = torch.full((N,), R, dtype=torch.int32, device="cuda")
    idx = torch.randint(0, N, (B,), device="cuda", generator=g)

    def gather():
        _lib.check(lib.vqa_gather_features(P(table), P(nbox), P(idx), P(V), P(nb), B, R, D, N, None), "gather")

    def gemm():
        _lib.check(lib.vqa_gemm_f32(0, 0, B * R, H, D, P(V), D, P(W), H, P(out), H, P(bias), None, 0, 1, None, 0, None), "gemm")

    def fused(which, byproduct, ptr=0):
        def f():
            if which is lib:
                lib.vqa_gemm_set_gather_ptr(ptr)
            _lib.check(which.vqa_gemm_f32_gather(B * R, H, D, P(table), D, P(idx), R, N, P(W), H, P(out2), H, P(bias),
                                                 P(V2) if byproduct else None, D, None), "fused")
        return f

    variants = [("plain gemm", gemm), ("gather pass", gather), ("pass + gemm", lambda: (gather(), gemm()))]
    if old is not None:
        variants += [("old fused, by-product", fused(old, True)), ("old fused, none", fused(old, False))]
    variants += [("new fused offsets, by-product", fused(lib, True)), ("new fused offsets, none", fused(lib, False)),
                 ("new fused pointers, by-product", fused(lib, True, 1)), ("new fused pointers, none", fused(lib, False, 1))]

    gather(); gemm(); torch.cuda.synchronize()
    for name, f in variants[3:]:                         # every fused form gives the pass + GEMM bits
        V2.fill_(float("nan")); out2.fill_(float("nan"))
        f(); torch.cuda.synchronize()
        assert torch.equal(out, out2), name
        assert "none" in name or torch.equal(V, V2), name
    times = {name: [] for name, _ in variants}
    for name, f in variants:
        timed(f, 3)
    for _ in range(args.runs):
        for name, f in variants:
            if touch:
                table.sum(); torch.cuda.synchronize()
            times[name].append(timed(f, args.calls))
    lib.vqa_gemm_set_gather_ptr(0)
    print("table of %d images (%.0f MB), %s: us per call, median of %d runs of %d calls" % (N, N * R * D * 4 / 1e6, label, args.runs, args.calls))
    for name, _ in variants:
        t = times[name]
        print("  %-32s median %7.1f  min %7.1f  max %7.1f | %s" % (name, statistics.median(t), min(t), max(t),
                                                                  " ".join("%.1f" % x for x in t)), flush=True)


bench_table(8192, "rows from HBM", False)
bench_table(256, "cache-resident, read once before every run", True)
