"""Host side of the micro-batched step (EngineCore.train_micro_steps; --accum_steps of both trainers); no GPU.

  * Discrimination, from the float64 oracle alone, on the exact cases tests/test_gpu_micro_steps.py holds the engine to
    (tests/micro_ref.ITEM2_CASES): the parameters after the three steps computed (a) correctly, (b) with clip + Adam after
    every micro-batch, (c) with every micro-batch scaled by 1 / its own rows instead of 1/G.  (b) and (c) must each sit at
    least 10 x the GPU test's parameter bound from (a) -- otherwise that test could pass an engine that does either.
    (c) is asserted where the micro-batches have unequal rows: n equal micro-batches scaled by 1 / own rows give exactly n
    times the gradient, and clip_by_global_norm + Adam do not see a common factor: the 16 + 16 cases cannot cover the
    scale, the 5 + 3, 20 + 12 and 264 + 8 cases do.
  * The row bookkeeping (engine_core.micro_plan) as a pure function.
  * --accum_steps parsing and the step counting of both trainers on stub models."""
import types

import numpy as np
import pytest

from tests import micro_ref as M

CASE_IDS = [c[0] for c in M.ITEM2_CASES]


def _distance(case, a, b):
    """worst max |a - b| over the trained variables, in units of the GPU test's bound for that variable"""
    return max(float(np.abs(a[n] - b[n]).max()) / M.param_tolerance(a[n]) for n in M.train_names(case)
               if not n.endswith("score/fc/biases"))


@pytest.mark.parametrize("name,model_type,shape,live_rows,clip", M.ITEM2_CASES, ids=CASE_IDS)
def test_the_wrong_steps_sit_ten_bounds_from_the_accumulated_step(name, model_type, shape, live_rows, clip):
    case = M.fusion_case(model_type, shape, live_rows=live_rows)
    trace = []
    a = M.adam_steps(case, "accumulated", clip=clip, trace=trace)
    if clip < 1.0:
        assert min(t["norm"] for t in trace) > 10 * clip            # clipping is active in every step
    b = M.adam_steps(case, "adam_each", clip=clip)
    c = M.adam_steps(case, "own_rows", clip=clip)
    db, dc = _distance(case, a, b), _distance(case, a, c)
    print("%s: Adam after every micro-batch %.1f bounds away, 1 / own rows %.1f" % (name, db, dc))
    assert db >= 10.0, db
    rows = {hi - lo for lo, hi, _ in case["cuts"]}
    if len(rows) > 1:             # (equal rows: a common factor n, which behind clip + Adam only Adam's epsilon sees)
        assert dc >= 10.0, dc


def test_accumulated_oracle_step_is_the_sum_of_the_micro_batch_gradients_scaled_by_their_rows_over_G():
    """the identity the engine implements: grad(concatenated batch) = sum_i rows_i / G * grad(micro-batch i), the slices'
    sum of squares included"""
    case = M.fusion_case("vlmap_answer", "small")
    p = case["p"]
    _, full, fs = M.loss_and_grads(case, p)
    G = case["B"]
    parts = [(M.loss_and_grads(case, p, lo, hi, T), (hi - lo) / G) for lo, hi, T in case["cuts"]]
    for n in M.train_names(case):
        want = sum(w * g[n] for (_, g, _), w in parts)
        assert np.abs(full[n] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), n
    sq = sum(float(((w * s[k]) ** 2).sum()) for (_, _, s), w in parts for k in s)
    assert abs(sq - sum(float((v ** 2).sum()) for v in fs.values())) <= 1e-12 * sq


def test_accumulated_oracle_step_is_the_cpu_baseline_step_on_the_whole_batch():
    """oracle/torch_ref.CpuTrainStep (f32, default clip) on the concatenated batch against this module's float64 step"""
    from oracle import torch_ref as TR
    case = M.fusion_case("vlmap_answer", "small")
    step = TR.CpuTrainStep(case["p"], case["table"], case["nbox"], case["am"], "vlmap_answer", lr=M.LR)
    for _ in range(M.STEPS):
        step(case["batch"], case["masks"])
    a = M.adam_steps(case, "accumulated")
    for n in M.train_names(case):
        if not n.endswith("score/fc/biases"):
            assert np.abs(step.P[n].detach().numpy() - a[n]).max() <= M.param_tolerance(a[n]), n


# ------------------------------------------------------------------------------------------------------ row bookkeeping
def test_micro_plan_prefix_sums_rank_offset_and_global_rows():
    from vqa_transfer_externaldata_amd.engine_core import micro_plan
    assert micro_plan([5, 3]) == ((0, 5), 8)
    assert micro_plan([7]) == ((0,), 7)
    assert micro_plan((128,) * 4) == ((0, 128, 256, 384), 512)
    # data parallel: rank 1 of 2, 2 micro-batches each, global batch 16: its rows follow its offset
    assert micro_plan([5, 3], row_offset=8, global_rows=16) == ((8, 13), 16)
    assert micro_plan([5, 3], row_offset=0, global_rows=16) == ((0, 5), 16)
    assert micro_plan([4], row_offset=3, global_rows=7) == ((3,), 7)
    for bad in ((), [0], [4, 0], [3, -1]):
        with pytest.raises(ValueError):
            micro_plan(bad)
    with pytest.raises(ValueError, match="do not fit"):
        micro_plan([5, 3], row_offset=9, global_rows=16)
    with pytest.raises(ValueError, match="do not fit"):
        micro_plan([5, 3], row_offset=-1)
    with pytest.raises(ValueError, match="do not fit"):
        micro_plan([5, 3], global_rows=7)


# ------------------------------------------------------------------------------------------------------ the trainers
def test_accum_steps_is_parsed_by_both_trainers():
    from vqa_transfer_externaldata_amd import pretrain_trainer, trainer
    assert trainer.parse_config([]).accum_steps == 1 and trainer.parse_config(["--accum_steps", "4"]).accum_steps == 4
    pp = pretrain_trainer.build_parser()
    assert pp.parse_args([]).accum_steps == 1 and pp.parse_args(["--accum_steps", "3"]).accum_steps == 3


class _StubVqaModel:
    """what vqa Trainer.run_train_step drives, recording the calls"""
    report = {"answer_train_loss": 0.0}
    device = "cpu"

    def __init__(self):
        self.calls, self._step = [], 0

    def set_batch(self, b):
        self.calls.append(("set_batch", b["id"]))

    def build(self):
        self.calls.append(("build",))

    def backward(self, reducer=None):
        self.calls.append(("backward",))

    def apply_gradients(self, lr):
        self.calls.append(("apply", lr))

    def train_micro_steps(self, batches, lr, allreduce=None, row_offset=0, global_rows=None):
        self.calls.append(("micro", tuple(b["id"] for b in batches), lr, row_offset, global_rows))


def _vqa_trainer(accum, world=1, rank=0, lr_decay=False):
    from vqa_transfer_externaldata_amd import dp, trainer

    class T(trainer.Trainer):
        def __init__(self):
            self.config = types.SimpleNamespace(lr_weight_decay=lr_decay, global_batch=None, shard_row_offset=0)
            self.world, self.rank, self.accum_steps, self.batch_size = world, rank, accum, 10
            self.model, self._allreduce = _StubVqaModel(), None
            self.global_step, self.learning_rate, self.drawn = 0, 1e-3, 0
            self._pending_train_batch = self._pending_global = None
            self.saved = []

        def _next(self, split):
            if self._pending_train_batch is not None:
                b, self._pending_train_batch = self._pending_train_batch, None
                self._set_global(self._pending_global)
                self._pending_global = None
                return b
            n_global = 10 - self.drawn % 2            # batches of 10 and 9 rows alternate
            self.drawn += 1
            self._set_global(n_global)
            lo, hi = dp.shard_bounds(n_global, self.rank, self.world) if self.world > 1 else (0, n_global)
            return {"id": self.drawn, "image_idx": np.zeros(hi - lo, np.int64)}

        def _report_values(self):
            return 0.5, {"answer_train_loss": 0.5}

        def save_checkpoint(self):
            self.saved.append(self.global_step)
    return T()


def test_vqa_trainer_counts_optimiser_steps_and_draws_n_batches_per_step():
    t = _vqa_trainer(accum=3)
    steps = [t.run_train_step(True) for _ in range(4)]
    assert [s[0] for s in steps] == [1, 2, 3, 4] and t.global_step == 4
    assert [s[1]["step"] for s in steps] == [1, 2, 3, 4]
    micro = [c for c in t.model.calls if c[0] == "micro"]
    assert len(micro) == 4 and len(t.model.calls) == 4                      # one call per optimiser step, nothing else
    assert [c[1] for c in micro] == [(1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)]      # every batch once, in order
    assert all(c[3] == 0 and c[4] is None for c in micro)                    # one process: the engine sums the rows
    # the learning-rate schedule reads optimiser steps: 10000 of them halve the rate, not 10000 batches
    t = _vqa_trainer(accum=3, lr_decay=True)
    t.global_step = 9999
    t.run_train_step(False)
    t.run_train_step(False)
    assert [c[2] for c in t.model.calls] == [1e-3, 5e-4]


def test_vqa_trainer_with_one_accum_step_is_the_step_it_was():
    t = _vqa_trainer(accum=1)
    t.run_train_step(False)
    t.run_train_step(False)
    assert [c[0] for c in t.model.calls] == ["set_batch", "build", "backward", "apply"] * 2
    assert t.global_step == 2


def test_vqa_trainer_places_a_ranks_micro_batches_in_the_global_batch():
    """data parallel: the N shards of a rank follow each other from the sum of their first rows, in a global batch of the
    sum of the N global batches -- ranks tile [0, G) without overlap"""
    from vqa_transfer_externaldata_amd import dp
    spans = []
    for rank in (0, 1):
        t = _vqa_trainer(accum=2, world=2, rank=rank)
        t.run_train_step(False)
        _, ids, _, row_offset, G = t.model.calls[0]
        assert G == 10 + 9 and ids == (1, 2)
        own = sum(hi - lo for lo, hi in (dp.shard_bounds(n, rank, 2) for n in (10, 9)))
        spans.append((row_offset, row_offset + own))
    assert spans == [(0, 10), (10, 19)]


def test_vqa_trainer_schedules_count_optimiser_steps(tmp_path):
    t = _vqa_trainer(accum=2)
    t.max_train_iter, t.train_average_iter, t.validation_step = 5, 2, 100
    t.heavy_summary_step, t.checkpoint_step, t._iters, t.val_average_iter = 2, 2, {}, 1
    t._summary_path = str(tmp_path / "summaries.jsonl")
    t.train()
    assert t.global_step == 5 and t.saved == [1, 3, 5]            # after optimiser steps 1, 3, 5 (s = 0, 2, 4)
    assert len([c for c in t.model.calls if c[0] == "micro"]) == 5 and t.drawn == 10 + 1     # + the batch drawn ahead


class _StubPretrainModel:
    device = "cpu"

    def __init__(self):
        self.calls, self.report, self._step = [], {"total_loss": 1.0}, 0

    def prepare(self, batch):
        return ("prepared", batch["id"])

    def build(self, prepared=None, defer_report=False):
        self.calls.append(("build", prepared[1]))

    def backward(self, reducer=None):
        self.calls.append(("backward",))

    def apply_gradients(self, lr):
        self.calls.append(("apply", lr))

    def train_micro_steps(self, prepared, lr, allreduce=None):
        self.calls.append(("micro", tuple(p[1] for p in prepared), lr))

    def finish_report(self):
        self.calls.append(("report",))


def _pretrain_trainer(accum, monkeypatch):
    import torch
    from vqa_transfer_externaldata_amd import pretrain_trainer
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)

    class T(pretrain_trainer.Trainer):
        def __init__(self):
            self.config = types.SimpleNamespace(lr_weight_decay=False)
            self.world, self.rank, self.accum_steps, self.batch_size = 1, 0, accum, 4
            self.model, self._allreduce = _StubPretrainModel(), None
            self.global_step, self.learning_rate, self.drawn = 0, 1e-3, 0

        def _next(self, split):
            self.drawn += 1
            return {"id": self.drawn}
    return T()


def test_pretrain_trainer_counts_optimiser_steps_and_draws_n_batches_per_step(monkeypatch):
    t = _pretrain_trainer(3, monkeypatch)
    steps = [t.run_train_step(True) for _ in range(3)]
    assert [s[0] for s in steps] == [1, 2, 3] and [s[1]["step"] for s in steps] == [1, 2, 3]
    micro = [c for c in t.model.calls if c[0] == "micro"]
    # step k runs the batch prepared ahead by step k-1, then two fresh ones; every batch once, in order
    assert [c[1] for c in micro] == [(1, 2, 3), (4, 5, 6), (7, 8, 9)]
    assert [c[0] for c in t.model.calls] == ["micro", "report"] * 3 and t.drawn == 10
    t = _pretrain_trainer(1, monkeypatch)
    t.run_train_step(False)
    assert [c[0] for c in t.model.calls] == ["build", "backward", "apply", "report"] and t.global_step == 1
