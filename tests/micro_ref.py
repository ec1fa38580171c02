"""Inputs and float64 references of the micro-batched step (EngineCore.train_micro_steps), shared by
tests/test_gpu_micro_steps.py and tests/test_micro_steps_host.py.  Nothing here touches a GPU.

A case is ONE global batch and how it is cut into micro-batches: rows (5 + 3, 16 + 16, 264 + 8) and a padded length per
micro-batch (the second one is shorter: its rows' lengths are capped at it; not for the bi-directional model, whose
LayerNorm over [T, H] blocks makes a row depend on its batch's padded length), with the dropout masks / noise of the whole
batch, from which every micro-batch takes its rows.  The reference is the float64 oracle on the concatenated batch:
oracle/torch_ref.loss_and_grads (oracle/bi_oracle.torch_loss_and_grads for the bi-directional model) and clip + Adam on
its gradients, the norm over the un-aggregated embedding slices.  Besides the correct step, `adam_steps` computes the two
wrong ones the host test must tell from it: Adam after every micro-batch, and every micro-batch scaled by 1 / its own rows.

Test infrastructure only (no product code imports it)."""
from __future__ import annotations

import numpy as np

from oracle import bi_oracle as BO
from oracle import torch_ref as TR
from oracle import vqa_oracle as O
from tests import encoder_routes_ref as E
from tests.bf16_ref import MED, SMALL
from tests.gpu_util import make_case, to64

SEED, STEPS = 21, 3
# The learning rate of the three steps: the one tests/test_gpu_fusion.py's parameter bound (below) was argued for.  At it a
# step that runs Adam after every micro-batch, or scales a micro-batch by 1 / its own rows, sits 11 to 19 times that bound
# from the correct one on these cases (tests/test_micro_steps_host.py asserts 10).
LR = 1e-3
# parameters after the steps, per variable: max |got - want| <= PARAM_ATOL + PARAM_RTOL max |want| and fewer than
# PARAM_OUTLIERS of the elements off by more than PARAM_OUTLIER_TOL -- the bounds of
# tests/test_gpu_fusion.test_train_steps_match_oracle_f32, which states them inline
PARAM_ATOL, PARAM_RTOL, PARAM_OUTLIER_TOL, PARAM_OUTLIERS = 4.5e-4, 1e-4, 1e-4, 0.02
MODEL_TYPES = ("vlmap_answer", "standard", "vlmap_answer_noc", "vlmap_answer_full", "vlmap_finetune")
# shape -> (dims, rows per micro-batch, R, padded length per micro-batch, images)
SHAPES = {"small": (SMALL, (5, 3), 6, (7, 5), 9),
          "med": (MED, (16, 16), 36, (14, 11), 64),
          # equal micro-batches cannot tell 1/G from 1 / own rows (n times the gradient: clip + Adam are scale-invariant)
          "med_uneven": (MED, (20, 12), 36, (14, 11), 64),
          # the question encoder's width, everything else tiny (tests/encoder_routes_ref.py): 264 rows take the
          # weight-stationary recurrence in both directions, 8 rows only forward (its backward needs more than 256)
          "h1024": (E.DIMS, (264, 8), E.R, (E.T, E.T - 1), E.N_IMG)}


# The cases of the oracle comparison (tests/test_gpu_micro_steps.py, item 2) = the inputs of the host test's discrimination:
# (id, model type, shape, live_rows, clip_norm).  Every model type at 5 + 3 and 16 + 16 rows; unequal rows at the MED
# dimensions; once with live_rows; once with a clip norm far below the gradient's norm of 3.8 (the MED cases clip at the
# default already: norm 38); the recurrence routing at H 1024.
ITEM2_CASES = [("%s-%s" % (mt, shape), mt, shape, False, O.CLIP_NORM) for shape in ("small", "med") for mt in MODEL_TYPES] + \
    [("vlmap_answer-med_uneven", "vlmap_answer", "med_uneven", False, O.CLIP_NORM),
     ("vlmap_answer-small-live_rows", "vlmap_answer", "small", True, O.CLIP_NORM),
     ("standard-small-live_rows", "standard", "small", True, O.CLIP_NORM),
     ("vlmap_answer-small-clip0.05", "vlmap_answer", "small", False, 0.05),
     ("vlmap_answer-h1024", "vlmap_answer", "h1024", False, O.CLIP_NORM)]


def param_tolerance(want):
    return PARAM_ATOL + PARAM_RTOL * float(np.abs(want).max())


def fusion_case(model_type, shape="small", live_rows=False):
    """dict: model_type, dims, R, N, p, table, nbox, am, batch and masks of the global batch (T = the longest micro-batch's),
    cuts = ((lo, hi, T_i), ...), live (per micro-batch int32 [T_i], or None)"""
    dims, rows, R, Ts, N = SHAPES[shape]
    if model_type in BO.MODEL_TYPES:
        # The bi-directional models normalise q_att_key and v_word_fc over the whole [T, H] block of a question
        # (layer_norm over every non-batch axis, as the reference's graph does): a row's output depends on the length its
        # batch is padded to, so rows padded to another T are not rows of the concatenated batch.  One T for these.
        Ts = (max(Ts),) * len(rows)
    B, T = sum(rows), max(Ts)
    if model_type in BO.MODEL_TYPES:
        rng = np.random.default_rng(SEED)
        p = O.perturb_ln_params(BO.init_params(rng, **dims), rng)
        table, nbox = O.make_table(rng, N, R, dims["D"], full_boxes=False)
        batch = O.make_batch(rng, B, T, dims["Vq"], dims["A"], N)
        am = O.make_answer_masks(rng, dims["A"], int(dims["A"] * 0.75), exist_all=False)
        masks = BO.make_masks(rng, B, R, T, dims["H"])
    else:
        p, table, nbox, batch, am, masks = make_case(SEED, model_type, B, R, T, N, dims)
    if shape == "h1024":      # states of order 0.1 instead of 1e-3 (tests/encoder_routes_ref._drawn)
        embed = O.scope_names(model_type)["embed"]
        p[embed] = np.random.default_rng(SEED + 1).standard_normal(p[embed].shape).astype(p[embed].dtype)
    cuts, lo = [], 0
    for r, Ti in zip(rows, Ts):
        cuts.append((lo, lo + r, Ti))
        ln = np.minimum(batch["q_intseq_len"][lo:lo + r], Ti)
        batch["q_intseq_len"][lo:lo + r] = ln
        batch["q_intseq"][lo:lo + r][np.arange(T)[None, :] >= ln[:, None]] = 0
        lo += r
    live = None
    if live_rows:             # every micro-batch's rows longest first, as input_ops_vqa.sort_by_length leaves a batch
        order, live = [], []
        for lo, hi, Ti in cuts:
            ln = batch["q_intseq_len"][lo:hi]
            o = np.argsort(-ln.astype(np.int64), kind="stable")
            order.append(lo + o)
            live.append((ln[o][None, :] > np.arange(Ti)[:, None]).sum(1).astype(np.int32))
        order = np.concatenate(order)
        batch = {k: np.ascontiguousarray(v[order]) for k, v in batch.items()}
        masks = {k: np.ascontiguousarray(v[order]) for k, v in masks.items()}
    return dict(model_type=model_type, dims=dims, R=R, N=N, B=B, T=T, p=p, table=table, nbox=nbox, am=am, batch=batch,
                masks=masks, cuts=tuple(cuts), live=live)


def rows_of(case, lo, hi, T):
    """(batch, masks) of the global rows [lo, hi) padded to T"""
    b = {k: np.ascontiguousarray(v[lo:hi]) for k, v in case["batch"].items()}
    b["q_intseq"] = np.ascontiguousarray(b["q_intseq"][:, :T])
    m = {k: np.ascontiguousarray(v[lo:hi]) for k, v in case["masks"].items()}
    if "word" in m:
        m["word"] = np.ascontiguousarray(m["word"][:, :T])
    return b, m


def micro_batches(case):
    """[(batch, masks)] of the case's micro-batches; a batch carries live_rows where the case has them"""
    out = []
    for i, (lo, hi, Ti) in enumerate(case["cuts"]):
        b, m = rows_of(case, lo, hi, Ti)
        if case["live"] is not None:
            b["live_rows"] = case["live"][i]
        out.append((b, m))
    return out


def train_names(case):
    mt = case["model_type"]
    return BO.train_var_names(case["p"], mt) if mt in BO.MODEL_TYPES else O.train_var_names(case["p"], mt)


def loss_and_grads(case, params, lo=0, hi=None, T=None):
    """float64: (loss, grads {name: array}, slices {embedding name: un-aggregated [rows, T, W]}) of the MEAN loss over the
    global rows [lo, hi)"""
    hi, T = case["B"] if hi is None else hi, case["T"] if T is None else T
    b, m = rows_of(case, lo, hi, T)
    mt = case["model_type"]
    args = (to64(params), to64(b), case["table"].astype(np.float64), case["nbox"], to64(case["am"]), to64(m))
    if mt in BO.MODEL_TYPES:
        loss, _, grads, slices = BO.torch_loss_and_grads(*args)
        names = train_names(case)
        return loss, grads, {k: v for k, v in slices.items() if k in names}
    loss, _, grads, dx = TR.loss_and_grads(*args, model_type=mt)
    return loss, grads, {O.scope_names(mt)["embed"]: dx}


def report(case, params):
    """(the scalar the optimiser minimises, report dict) of the float64 forward on the whole batch"""
    mt = case["model_type"]
    args = (to64(params), to64(case["batch"]), case["table"].astype(np.float64), case["nbox"], to64(case["am"]),
            to64(case["masks"]))
    if mt in BO.MODEL_TYPES:
        loss, rep, _, _ = BO.forward(*args)
        return loss, rep
    loss, rep, _, _, _ = O.forward(*args, mt)
    return loss, rep


def clip_adam(params, grads, slices, names, state, lr, clip):
    """clip_by_global_norm(clip) + Adam (oracle/vqa_oracle.clip_adam_step's arithmetic) in place on float64 `params`, for
    any number of embedding tables; returns the global norm"""
    norm = BO.global_norm(grads, names, slices)
    scale = clip / max(norm, clip)
    state["step"] += 1
    t = state["step"]
    lr_t = lr * np.sqrt(1 - O.ADAM_B2 ** t) / (1 - O.ADAM_B1 ** t)
    for n in names:
        g = grads[n] * scale
        m = state["m"].setdefault(n, np.zeros_like(params[n]))
        v = state["v"].setdefault(n, np.zeros_like(params[n]))
        m[...] = O.ADAM_B1 * m + (1 - O.ADAM_B1) * g
        v[...] = O.ADAM_B2 * v + (1 - O.ADAM_B2) * g * g
        params[n] -= lr_t * m / (np.sqrt(v) + O.ADAM_EPS)
    return norm


def adam_steps(case, mode="accumulated", steps=STEPS, lr=LR, clip=O.CLIP_NORM, trace=None):
    """float64 parameters after `steps` optimiser steps on the case's global batch.
    mode "accumulated": the correct step -- the gradient of the concatenated batch, one clip + Adam;
         "adam_each":   WRONG -- clip + Adam after every micro-batch (on its gradient scaled by 1/G);
         "own_rows":    WRONG -- the micro-batches' gradients summed, each scaled by 1 / its own rows instead of 1/G.
    trace: a list that receives per step (grads, slices, norm, loss, report) of the correct step"""
    p = to64(case["p"])
    names, state, G = train_names(case), O.new_opt_state(), case["B"]
    for _ in range(steps):
        if mode == "accumulated":
            loss, grads, slices = loss_and_grads(case, p)
            if trace is not None:
                rep = report(case, p)
            norm = clip_adam(p, grads, slices, names, state, lr, clip)
            if trace is not None:
                trace.append(dict(grads=grads, slices=slices, norm=norm, loss=rep[0], report=rep[1]))
            continue
        parts = [loss_and_grads(case, p, lo, hi, Ti) + (hi - lo,) for lo, hi, Ti in case["cuts"]]
        if mode == "adam_each":
            for i, (lo, hi, Ti) in enumerate(case["cuts"]):
                if i:         # the parameters moved: this micro-batch's gradient is taken where they are now
                    parts[i] = loss_and_grads(case, p, lo, hi, Ti) + (hi - lo,)
                _, g, s, r = parts[i]
                clip_adam(p, {k: v * (r / G) for k, v in g.items()}, {k: v * (r / G) for k, v in s.items()}, names, state,
                          lr, clip)
        elif mode == "own_rows":
            grads = {k: sum(g[k] for _, g, _, _ in parts) for k in parts[0][1]}
            # the norm's slices: every micro-batch's own, side by side (zero-padded to the longest)
            T = case["T"]
            pad = lambda a: np.pad(a, ((0, 0), (0, T - a.shape[1]), (0, 0)))
            slices = {k: np.concatenate([pad(s[k]) for _, _, s, _ in parts]) for k in parts[0][2]}
            clip_adam(p, grads, slices, names, state, lr, clip)
        else:
            raise ValueError(mode)
    return p
