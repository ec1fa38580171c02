"""What the two train-step engines (fusion.FusionEngine, pretrain.PretrainEngine) share, and nothing model-specific:
the flat parameter / gradient / Adam buffers carved from one table, their checkpoint half, clip_by_global_norm + Adam
on them, the phased backward that starts a bucket's reduction as soon as its gradients are complete, and the growth of
the kernel workspace.

Flat buffers (all fp32; every variable padded to a multiple of 4 floats, in the order of the engine's table):
  train_flat, m_flat, v_flat = parameters and Adam moments
  grad_flat                  = same layout + 4 trailing floats; slot 0 of the tail carries the un-aggregated sum of
                               squares of the scatter-added tables' slices, so that ONE all-reduce moves gradients and
                               that scalar under data parallel
  acc_flat                   = grad_flat's layout, tail included; exists only once a step of more than one micro-batch
                               has run (train_micro_steps): the sum of the micro-batches' grad_flat
An engine sets `clip_norm`, implements `_backward_phases(bits)` and declares which buckets of grad_flat are complete
after which phase (`_set_schedule`).  For train_micro_steps it also implements `_micro_rows`, `_micro_open`,
`_micro_forward`, `_micro_stats` and `_micro_close`.
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


def micro_plan(rows, row_offset=0, global_rows=None):
    """((first global row of every micro-batch, ...), G) for micro-batches of `rows` rows each, run one after the other:
    a micro-batch is a rank in time, so micro-batch i starts at row_offset + the rows before it.  G, the global batch every
    gradient is scaled by, is their sum -- or global_rows under data parallelism, where row_offset is the first global
    row of this rank and its rows must fit below G."""
    rows = [int(r) for r in rows]
    if not rows:
        raise ValueError("train_micro_steps needs at least one micro-batch")
    if min(rows) <= 0:
        raise ValueError("a micro-batch without rows cannot run the step (rows: %s)" % (rows,))
    row_offset, local = int(row_offset), sum(rows)
    G = local if global_rows is None else int(global_rows)
    if row_offset < 0 or row_offset + local > G:
        raise ValueError("rows [%d, %d) of this step do not fit the global batch of %d" % (row_offset, row_offset + local, G))
    starts = tuple(row_offset + sum(rows[:i]) for i in range(len(rows)))
    return starts, G


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
        self.acc_flat, self._dense_lo = None, dense_lo        # train_micro_steps allocates acc_flat on first use
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

    def optimizer_step(self, lr, accumulated=False):
        """clip_by_global_norm(clip_norm) + Adam on the flat buffers.  The norm uses the dense gradients of every
        variable behind the scatter-added tables plus those tables' un-aggregated slices (tail slot), as
        tf.clip_by_global_norm does for IndexedSlices.  accumulated: the gradients are acc_flat's (train_micro_steps)."""
        lib, st = self.lib, self._stream()
        sumsq, adam = (self._acc_sumsq_ptrs + (st,), self._acc_adam_ptrs) if accumulated else \
            (self._sumsq_args(st), self._adam_ptrs)
        _lib.check(lib.vqa_sumsq(*sumsq), "vqa_sumsq")
        self.step_count += 1
        t = self.step_count
        lr_t = lr * math.sqrt(1.0 - ADAM_B2 ** t) / (1.0 - ADAM_B1 ** t)
        _lib.check(lib.vqa_clip_adam(*adam, float(self.clip_norm), lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, st),
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

    # ------------------------------------------------------------------ micro-batched step
    def _ensure_acc_flat(self):
        """acc_flat (grad_flat's layout, the 4 tail floats included) and the norm / update arguments that read it"""
        if self.acc_flat is None:
            n, lo = self.n_train, self._dense_lo
            self.acc_flat = torch.zeros(n + 4, dtype=torch.float32, device=self.grad_flat.device)
            P = lambda t: C.c_void_p(t.data_ptr())
            self._acc_sumsq_ptrs = (P(self.acc_flat[lo:n]), n - lo, P(self.acc_flat[n:])) + self._sumsq_ptrs[3:]
            self._acc_adam_ptrs = (self._adam_ptrs[0], P(self.acc_flat)) + self._adam_ptrs[2:]
        return self.acc_flat

    def train_micro_steps(self, micro, lr, allreduce=None, row_offset=0, global_rows=None, global_valid=None):
        """ONE optimiser step on the gradient of the concatenation of the micro-batches `micro`: a micro-batch is a rank
        in time.  micro: a sequence of n >= 1 dicts {"batch": ..., + what the engine's train_step takes for that batch
        (explicit keep masks / noise, or dropout=(seed, step))}; row counts (and the fusion model's T) may differ, the
        workspace only grows.  G = the sum of their rows (global_rows under data parallelism, with row_offset = this
        rank's first global row).  Micro-batch i runs forward and backward scaled by 1/G with its dropout streams at
        global row row_offset + rows before it; after its backward acc_flat += grad_flat, tail floats included, in
        micro-batch order (the first one is copied).  After the last: `allreduce` ONCE on the whole of acc_flat (a
        bucketed reducer gets it as a single bucket: its overlap with the backward phases is given up, there is one
        collective per optimiser step, not per micro-batch), then the norm and clip + Adam read acc_flat, and step_count
        advances by one.  The report of the step is the global batch's (the engines' report functions).
        n == 1 is train_step launch for launch: no accumulation pass, acc_flat is neither made nor touched, and a
        bucketed reducer keeps its overlap.  Seeded and explicit dropout cannot be mixed inside one step (ValueError), and
        a micro-batched step is never a graph replay (train_step_graph refuses a sequence of batches).
        global_valid: the pre-training engine's (object, attribute) valid-entry counts of the global batch, as for its
        train_step; None: summed from the micro-batches."""
        micro = [dict(m) for m in micro]
        starts, G = micro_plan([self._micro_rows(m) for m in micro], row_offset, global_rows)
        if len({m.get("dropout") is not None for m in micro}) > 1:
            raise ValueError("seeded (dropout=(seed, step)) and explicit dropout cannot be mixed inside one optimiser step")
        ctx = self._micro_open(micro, G, global_rows is not None, allreduce, global_valid)
        try:
            if len(micro) == 1:
                self._micro_forward(micro[0], starts[0], G, ctx)
                self._backward_and_step(lr, allreduce)
                return
            from . import ops
            acc = self._ensure_acc_flat()
            for i, (m, start) in enumerate(zip(micro, starts)):
                self._micro_forward(m, start, G, ctx)
                self.backward()
                stats = self._micro_stats()
                if i == 0:                    # 0 + g = g: the first micro-batch is copied, the others are added in order
                    acc.copy_(self.grad_flat)
                    if getattr(self, "_micro_acc_stats", None) is None or self._micro_acc_stats.numel() != stats.numel():
                        self._micro_acc_stats = torch.zeros_like(stats)
                    self._micro_acc_stats.copy_(stats)
                else:
                    ops.add_inplace(acc, self.grad_flat)
                    self._micro_acc_stats.add_(stats)
            if allreduce is not None:
                if hasattr(allreduce, "start"):
                    allreduce.start(acc)
                    allreduce.finish()
                else:
                    allreduce(acc)
            self.optimizer_step(lr, accumulated=True)
            self._micro_report = {"stats": self._micro_acc_stats, "G": G, "dp": global_rows is not None,
                                  "group": getattr(allreduce, "group", None), "mean": None}
        finally:
            self._micro_close(ctx)
