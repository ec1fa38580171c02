"""What the two train-step engines (fusion.FusionEngine, pretrain.PretrainEngine) share, and nothing model-specific:
the flat parameter / gradient / Adam buffers carved from one table, their checkpoint half, clip_by_global_norm + Adam
on them, the phased backward that starts a bucket's reduction as soon as its gradients are complete, and the growth of
the kernel workspace.

Flat buffers (all fp32; every variable padded to a multiple of 4 floats, in the order of the engine's table):
  train_flat, m_flat, v_flat = parameters and Adam moments
  grad_flat                  = same layout + 4 trailing floats; slot 0 of the tail carries the un-aggregated sum of
                               squares of the scatter-added tables' slices, so that ONE all-reduce moves gradients and
                               that scalar under data parallel
An engine sets `clip_norm`, implements `_backward_phases(bits)` and declares which buckets of grad_flat are complete
after which phase (`_set_schedule`).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8     # tf.train.AdamOptimizer defaults


def pad4(n):
    return (n + 3) // 4 * 4


def carve(names, shapes):
    """({name: (offset, count)}, total floats): the variables `names` in this order, each padded to 4 floats"""
    off, table = 0, {}
    for n in names:
        cnt = int(np.prod(shapes[n]))
        table[n] = (off, cnt)
        off += pad4(cnt)
    return table, off


def phase_schedule(bucket_phases, buckets):
    """((phase bit, ((lo, hi), ...)), ...) from `buckets` in the order their reductions start and
    bucket_phases = ((phase bit, how many of them start after it), ...)"""
    it = iter(buckets)
    out = tuple((bit, tuple(next(it) for _ in range(cnt))) for bit, cnt in bucket_phases)
    assert next(it, None) is None, "a bucket that no phase starts"
    return out


class EngineCore:
    def _alloc_flat(self, table, n_train, shapes, dense_lo, device):
        """The flat buffers for `table` (carve) and the `params` / `grads` views of its variables.  dense_lo: where the
        dense part of grad_flat begins (the scatter-added tables lie before it; their norm travels in the tail)."""
        self._flat_tab, self.n_train = table, n_train
        f32 = dict(dtype=torch.float32, device=device)
        self.train_flat = torch.zeros(n_train, **f32)
        self.grad_flat = torch.zeros(n_train + 4, **f32)      # tail slot 0: un-aggregated slice sum of squares
        self.m_flat, self.v_flat = torch.zeros(n_train, **f32), torch.zeros(n_train, **f32)
        self.norm_sq = torch.zeros(4, **f32)
        self.sumsq_ws = torch.zeros(int(_lib.load().vqa_sumsq_workspace_floats(n_train)) + 4, **f32)
        self.params, self.grads = {}, {}
        for n, (off, cnt) in table.items():
            self.params[n] = self.train_flat[off:off + cnt].view(shapes[n])
            self.grads[n] = self.grad_flat[off:off + cnt].view(shapes[n])
        P = lambda t: C.c_void_p(t.data_ptr())
        self._sumsq_ptrs = (P(self.grad_flat[dense_lo:n_train]), n_train - dense_lo, P(self.grad_flat[n_train:]),
                            P(self.norm_sq), P(self.sumsq_ws), self.sumsq_ws.numel())
        self._adam_ptrs = (P(self.train_flat), P(self.grad_flat), P(self.m_flat), P(self.v_flat), n_train, P(self.norm_sq))

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """Flat name -> CPU tensor archive with the reference's variable names, the Adam slots of every trained
        variable (`<var>/Adam`, `<var>/Adam_1`) and global_step, the analogue of tf.train.Saver's checkpoint."""
        out = {n: p.detach().cpu().clone() for n, p in self.params.items()}
        for n, (off, cnt) in self._flat_tab.items():
            out[n + "/Adam"] = self.m_flat[off:off + cnt].view(self.params[n].shape).cpu().clone()
            out[n + "/Adam_1"] = self.v_flat[off:off + cnt].view(self.params[n].shape).cpu().clone()
        out["global_step"] = torch.tensor(self.step_count, dtype=torch.int64)
        return out

    def _load_optimizer_state(self, sd):
        """Adam moments and the step count (beta powers) of a state_dict (tensors or arrays), where it has them"""
        for n, (off, cnt) in self._flat_tab.items():
            if n + "/Adam" in sd:
                self.m_flat[off:off + cnt].copy_(torch.as_tensor(sd[n + "/Adam"]).reshape(-1))
                self.v_flat[off:off + cnt].copy_(torch.as_tensor(sd[n + "/Adam_1"]).reshape(-1))
        if "global_step" in sd:
            self.step_count = int(sd["global_step"])

    # ------------------------------------------------------------------ step pieces
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _ensure_workspace(self, workspace_bytes, dims, rejected, before_grow=None):
        """The workspace `dims` need by the engine's *_workspace_bytes entry point; it only grows.  before_grow: called
        before an existing workspace is replaced (whatever holds its addresses lets go)."""
        need = int(workspace_bytes(C.byref(dims)))
        if need <= 0:
            raise _lib.VqaHotError(rejected)
        if self.workspace is None or need > self.workspace.numel():
            if before_grow is not None and self.workspace is not None:
                before_grow()
            self.workspace = torch.zeros(need, dtype=torch.uint8, device=self.device)

    def _set_schedule(self, schedule):
        """schedule (phase_schedule): the buckets become views of grad_flat, built once per layout"""
        self._schedule = tuple((bit, tuple(self.grad_flat[lo:hi] for lo, hi in slices)) for bit, slices in schedule)

    def backward(self, reducer=None):
        """All gradients into grad_flat.  With a bucketed `reducer` (dp.BucketedAllReduce) the dependency-ordered
        phases are enqueued one by one and each finished bucket's all-reduce is started right away, so it overlaps the
        next phase."""
        if reducer is None:
            self._backward_phases(15)
            return
        for bit, buckets in self._schedule:
            self._backward_phases(bit)
            for b in buckets:
                reducer.start(b)
        reducer.finish()

    def _sumsq_args(self, stream):
        """vqa_sumsq's arguments: the dense part of grad_flat plus the tail slot into norm_sq"""
        return self._sumsq_ptrs + (stream,)

    def optimizer_step(self, lr):
        """clip_by_global_norm(clip_norm) + Adam on the flat buffers.  The norm uses the dense gradients of every
        variable behind the scatter-added tables plus those tables' un-aggregated slices (tail slot), as
        tf.clip_by_global_norm does for IndexedSlices."""
        lib, st = self.lib, self._stream()
        _lib.check(lib.vqa_sumsq(*self._sumsq_args(st)), "vqa_sumsq")
        self.step_count += 1
        t = self.step_count
        lr_t = lr * math.sqrt(1.0 - ADAM_B2 ** t) / (1.0 - ADAM_B1 ** t)
        _lib.check(lib.vqa_clip_adam(*self._adam_ptrs, float(self.clip_norm), lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, st),
                   "vqa_clip_adam")

    def _backward_and_step(self, lr, allreduce):
        """train_step behind the forward: `allreduce` is a bucketed reducer (overlapped with the backward phases), any
        callable on grad_flat, or None"""
        if allreduce is not None and hasattr(allreduce, "start"):
            self.backward(reducer=allreduce)
        else:
            self.backward()
            if allreduce is not None:
                allreduce(self.grad_flat)
        self.optimizer_step(lr)
