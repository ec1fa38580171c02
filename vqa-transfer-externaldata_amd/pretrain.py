"""cfg-5 pre-training ("task discovery") model on MI355X: the counterpart of
vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp.py:54-94, 323-609, 675-706.

Spatial attention over the 36 regions for n = 5 annotated boxes per image, blank-fill (GRU over the
caption with a blank) and word-set conditioned heads for objects and attributes, all four heads
sharing pooled_linear_l / q_linear_l / joint_fc / classifier, softmax-CE over the obj3000+attr1000 answers with
top-1 / top-5 accuracy.  LayerNorm variables of those shared fc_layer scopes: ONE per scope, trained by every call
site (`ln_shared=True`, the default: TF 1.x zeroes a string-named scope's sub-scope counts when it exits, so the
un-scoped layer_norm is `LayerNorm` again at the next call site and AUTO_REUSE shares it -- DESIGN.md section 2), or one per
call site (`LayerNorm`, `LayerNorm_1`, ... in graph build order) when a checkpoint carries those names:
`ln_shared_in(names)` decides and `load_state_dict` switches the engine over.  Forward and the hand-derived backward are
ONE C call each (vqa_pretrain_forward / vqa_pretrain_backward, csrc/pretrain_model.hip: every kernel of the
pass is enqueued from C++, the workspace is carved from the dims, no torch op runs inside the step); the
effective batch is B*n rows and the x n tile of V_ft / spatial_ft that the reference materialises (:324-333)
never exists: the attention kernels take `rep = n` queries per memory and v_linear_v of the (identical) tiles
is computed once per image.

The enwiki-context models of the paper's pipeline (vlmap_memft/model_vlmap_bf_or_wordset_enwiki_withatt_sp.py and
model_vlmap_bf_enwiki_withatt_sp.py) are the same engine with another head set (`heads`, MODEL_HEADS): per category an
enwiki head (enwiki_map embedding of the answer's context -> encode_L_enwiki GRU -> the shared fusion MLP) beside the
blank-fill and (optionally) word-set heads.  Those run on vqa_pretrain_ext_forward / _backward_phases; the cfg-5 head
set keeps the vqa_pretrain_* calls.

The "no composition" models (vlmap_memft/model_vlmap_noc_bf_or_wordset_withatt_sp.py, its copy
model_vlmap_nocarch_bf_or_wordset_withatt_sp.py and model_vlmap_noc_bf_or_enwiki_withatt_sp.py; NOC_MODEL_HEADS) are
the engine with `noc=True`: per head, instead of joint_fc(v_linear_l * l_linear_l) -> classifier, two branches
joint_v -> classifier_v on v_linear_l and joint_l -> classifier_l on l_linear_l; a blank-fill head's loss is the CE of
v_logit + l_logit (SUM), a word-set / enwiki head has one CE per branch (SPLIT, NOC_LOSS_MODE).  Those run on
vqa_pretrain_noc_forward / _backward_phases, and their checkpoints feed export_noc_word_weights -> vlmap_answer_noc.

The adapted-memory model (vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp_adapt.py; ADAPT_MODEL_HEADS) is the engine
with `adapt=True`: v_adapt = fc_layer(V_ft, 1024, LayerNorm over the [36, 1024] block, ReLU) (:346-350, :442-446) is what
the attention pools (:365-367, :461-463), so pooled_linear_l is [H, H] -- the only pre-training checkpoint
vlmap_answer_adapt can transfer its heads from.  It runs on vqa_pretrain_adapt_forward / _backward_phases; the FC is
computed once per image and once for both categories, and its gradients complete in backward phase 8.

Dropout: explicit uint8 keep-masks from make_keep_masks(B, seed, step) (the default), or `dropout=(seed, step)`: the same
bits computed inside the attention and LayerNorm kernels that consume them (vqa_pretrain_*_ex with a vqa_pretrain_keep_t;
DESIGN.md section 7), no mask tensor, bit for bit the same step.  keep_offsets() is the one copy of the stream layout.

Precision: f32, or opt-in `precision="bf16"` (the routed head layers on the bf16 matrix unit) and on top of it
`features="bf16"` (the region features at rest as bf16: table, gathered rows and what the attention kernels read) and
`encoder="bf16"` (both sequence encoders on the bf16 matrix unit: their five products and the per-step recurrence).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .engine_core import EngineCore, carve, phase_schedule

TOP_K = 5
KINDS = ("obj", "attr")
KEEP_ATT, KEEP_JOINT = 0.8, 0.5
CLIP_NORM = 20.0
NO_GRAD_VARS = ("V_GloVe/embed_map", "LearnAnswerGloVe/embed_map")      # created for export only
SPARSE_VARS = ("wordset_map/learn", "L_GloVe/embed_map", "enwiki_map/learn")   # IndexedSlices gradients (if present)
# Order of the dense variables in the flat buffers = the order in which the phases of vqa_pretrain_backward_phases
# complete their gradients, so every data-parallel bucket is one contiguous range:
#   [wordset_map | L_GloVe, enwiki_map (phase 4) | GRUs (phase 2) | stacked heads (phase 1) |
#    spatial attention, wordset_ft, v_adapt (phase 8: v_adapt's gradients need the attention backward of both categories) |
#    tail]
PHASE_SCOPES = (("encode_L_blank/", "encode_L_enwiki/"),
                ("classifier/", "joint_fc/", "pooled_linear_l/", "q_linear_l/", "classifier_v/", "classifier_l/", "joint_v/",
                 "joint_l/"),
                ("spat_att/", "spat_q_linear_v/", "spat_v_linear_v/", "wordset_ft/", "v_adapt/"))
# PretrainEngine.backward(reducer=...) (engine_core; vlmap_memft/trainer.py:129-137: optimize_loss over every variable):
# (phase bit, how many of flat_layout's buckets start their reduction after it) -- after 1 the stacked heads [b2:b3]
# (50+ MB, reduced under the back-propagation through time); after 2 the GRUs [b1:b2] (under the dx GEMM + embedding
# scatter-add); after 4 L_GloVe (+ enwiki_map) [b0:b1] (under the spatial-attention backward); after 8 wordset_map [:b0],
# then the spatial attention / wordset_ft / v_adapt gradients with the tail [b3:]: only these small ones are exposed.
# Nothing is zeroed before the phases: the C side clears the scatter-added tables.
BUCKET_PHASES = ((1, 1), (2, 1), (4, 1), (8, 2))
# head set per model type: blank fill, word set, enwiki context (in TF build order; head 2 r + k of the type of rank r
# and category k owns LayerNorm slot 2 r + k of the shared fusion scopes when they are not shared)
MODEL_HEADS = {"vlmap_bf_or_wordset_withatt_sp": ("bf", "ws"),
               "vlmap_bf_or_wordset_enwiki_withatt_sp": ("bf", "ws", "ew"),
               "vlmap_bf_enwiki_withatt_sp": ("bf", "ew")}
CFG5_HEADS = ("bf", "ws")
TASK_NAMES = {"bf": "blank_fill", "ws": "wordset", "ew": "enwiki"}
# the enwiki heads' joint keep-masks are drawn from counters at and above this one: disjoint from the cfg-5 stream
EW_MASK_COUNTER = 1 << 62
# "no composition" models: head set per model type (the nocarch file is a byte-identical copy of the noc one) and the
# loss of each head type -- 'sum': one CE of v_logit + l_logit, 'split': one CE of each branch
NOC_MODEL_HEADS = {"vlmap_noc_bf_or_wordset_withatt_sp": ("bf", "ws"),
                   "vlmap_nocarch_bf_or_wordset_withatt_sp": ("bf", "ws"),
                   "vlmap_noc_bf_or_enwiki_withatt_sp": ("bf", "ew")}
NOC_LOSS_MODE = {"bf": "sum", "ws": "split", "ew": "split"}
# the adapted-memory model (the attention pools v_adapt [R, H] instead of the features [R, D])
ADAPT_MODEL_HEADS = {"vlmap_bf_or_wordset_withatt_sp_adapt": ("bf", "ws")}
# the l branch's joint keep-masks of the noc heads: counters from here up, below EW_MASK_COUNTER (the v branch reuses the
# bf / ws / ew joint streams, which keep their bits)
NOC_L_MASK_COUNTER = 1 << 61


def ln_name(scope, idx):
    return scope + ("/LayerNorm" if idx == 0 else "/LayerNorm_%d" % idx)


def ln_shared_in(names):
    """True when the variable names are those of the shared-LayerNorm graph (no `<scope>/LayerNorm_<k>/...`)."""
    return not any("/LayerNorm_" in k for k in names)


def head_mask(heads):
    """VQA_PT_HEAD_* bits of a head set"""
    return sum({"bf": _lib.PT_HEAD_BF, "ws": _lib.PT_HEAD_WS, "ew": _lib.PT_HEAD_EW}[h] for h in heads)


def report_keys(heads=CFG5_HEADS, noc=False):
    """the model's report keys: per category, per head type <kind>_<task>_{loss,acc,top_5_acc} (a SPLIT head of a noc
    model: <kind>_<task>_v_{...} then <kind>_<task>_l_{...}); then total_loss"""
    return ["%s_%s%s_%s" % (k, TASK_NAMES[h], b, m) for k in KINDS for h in heads
            for b in (("_v", "_l") if noc and NOC_LOSS_MODE[h] == "split" else ("",))
            for m in ("loss", "acc", "top_%d_acc" % TOP_K)] + ["total_loss"]


def variable_shapes(Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, heads=CFG5_HEADS, n_ctx=None, noc=False,
                    adapt=False):
    """Variables of the model with head set `heads` (n_ctx: the enwiki context vocabulary, with 'ew'); noc: joint_v /
    joint_l and classifier_v / classifier_l instead of joint_fc and classifier; adapt: the v_adapt scope (two call
    sites: object, attribute) and a pooled_linear_l that reads the H-wide pooled v_adapt."""
    heads = tuple(heads)
    s = {"wordset_map/learn": (n_ws, W), "V_GloVe/embed_map": (Vq, W), "L_GloVe/embed_map": (Vq, W),
         "LearnAnswerGloVe/embed_map": (A, W)}
    if "ew" in heads:
        s["enwiki_map/learn"] = (int(n_ctx), W)

    def fc(scope, fin, fout, n_ln):
        s[scope + "/fc/weights"] = (fin, fout)
        s[scope + "/fc/biases"] = (fout,)
        for i in range(min(n_ln, 1) if ln_shared else n_ln):
            s[ln_name(scope, i) + "/beta"] = (fout,)
            s[ln_name(scope, i) + "/gamma"] = (fout,)

    fc("spat_v_linear_v", 6, H, 2)
    fc("spat_q_linear_v", 6, H, 2)
    fc("spat_att/compute/score", H, 1, 0)
    s["encode_L_blank/rnn/gru_cell/gates/kernel"] = (W + H, 2 * H)
    s["encode_L_blank/rnn/gru_cell/gates/bias"] = (2 * H,)
    s["encode_L_blank/rnn/gru_cell/candidate/kernel"] = (W + H, H)
    s["encode_L_blank/rnn/gru_cell/candidate/bias"] = (H,)
    if "ew" in heads:
        s["encode_L_enwiki/rnn/gru_cell/gates/kernel"] = (W + H, 2 * H)
        s["encode_L_enwiki/rnn/gru_cell/gates/bias"] = (2 * H,)
        s["encode_L_enwiki/rnn/gru_cell/candidate/kernel"] = (W + H, H)
        s["encode_L_enwiki/rnn/gru_cell/candidate/bias"] = (H,)
    if adapt:
        fc("v_adapt", D, H, 2)
    fc("pooled_linear_l", H if adapt else D, H, 2 * len(heads))
    fc("q_linear_l", H, H, 2 * len(heads))
    for scope in (("joint_v", "joint_l") if noc else ("joint_fc",)):
        fc(scope, H, 2 * H, 2 * len(heads))
    if "ws" in heads:
        fc("wordset_ft", W, H, 2)
    for scope in (("classifier_v", "classifier_l") if noc else ("classifier",)):
        fc(scope, 2 * H, A, 0)
    return s


def init_random_params(rng, Vq, n_ws, A, W=300, D=2048, H=1024, ln_shared=True, heads=CFG5_HEADS, n_ctx=None, noc=False,
                       adapt=False):
    """Random-init weights of the architecture (Xavier-uniform FCs, GRU gate bias 1, LN gamma 1,
    embeddings U(-0.01, 0.01); GloVe vectors are download-only)."""
    p = {}
    for n, shp in variable_shapes(Vq, n_ws, A, W, D, H, ln_shared, heads, n_ctx, noc, adapt).items():
        if n.endswith("/weights") or n.endswith("/kernel"):
            lim = np.sqrt(6.0 / (shp[0] + shp[1]))
            p[n] = rng.uniform(-lim, lim, size=shp).astype(np.float32)
        elif n.endswith("gates/bias") or n.endswith("/gamma"):
            p[n] = np.ones(shp, np.float32)
        elif n.endswith("embed_map") or n.endswith("/learn"):
            p[n] = rng.uniform(-0.01, 0.01, size=shp).astype(np.float32)
        else:
            p[n] = np.zeros(shp, np.float32)
    return p


def _length_sort(batch, len_key, tok_key):
    """{'perm', 'inv', 'live_rows'} over the 2*B*n rows of both categories (object rows first), ordered by the lengths
    '<kind>_blank_fill/<len_key>' (longest first); live_rows[t] = #rows longer than t, t below the padded length of
    '<kind>_blank_fill/<tok_key>'.  None when the batch does not carry the lengths as host arrays."""
    keys = [k + "_blank_fill/" + len_key for k in KINDS]
    if any(k not in batch or torch.is_tensor(batch[k]) for k in keys):
        return None
    lens = np.concatenate([np.asarray(batch[k]).reshape(-1) for k in keys]).astype(np.int64)
    L = int(np.asarray(batch[KINDS[0] + "_blank_fill/" + tok_key]).shape[-1])
    perm = np.argsort(-lens, kind="stable")
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    sl = np.clip(lens[perm], 0, L)
    return {"perm": perm, "inv": inv, "live_rows": (sl[None, :] > np.arange(L)[:, None]).sum(1).astype(np.int32)}


def add_length_sort(batch):
    """Host-side: the blank-fill captions of both categories are encoded as ONE batch of 2*B*n rows (object rows first).
    This adds 'blank_fill/sort' = the permutation that orders those rows by length (longest first), its inverse and
    live_rows[t] = #captions longer than t.  The engine then embeds / encodes the captions in that order, runs every GRU
    step on the live prefix only, and un-permutes the final states."""
    srt = _length_sort(batch, "blanks_len", "blanks")
    if srt is None:
        return batch
    batch["blank_fill/sort"] = srt
    return add_context_sort(batch)


def add_context_sort(batch):
    """The enwiki contexts of both categories the same way: 'enwiki_context/sort' = permutation (longest first), inverse
    and live_rows over the 2*B*n context rows, so that encode_L_enwiki also runs on the live prefix only."""
    srt = _length_sort(batch, "enwiki_context_len", "enwiki_context")
    if srt is not None:
        batch["enwiki_context/sort"] = srt
    return batch


# The C parameter structs: per struct type its members as (member, source).  A source is a variable name (a plain
# pointer), (scope, LayerNorm slots) for an fc_layer scope ("nh": one slot per head), or a nested struct type.  A table
# that lacks a variable is a KeyError, except for the members only some head sets have (_OPTIONAL: NULL then).
_GRU, _EGRU = "encode_L_blank/rnn/gru_cell/", "encode_L_enwiki/rnn/gru_cell/"
_TRUNK = (("wordset_map", "wordset_map/learn"), ("l_glove", "L_GloVe/embed_map"),
          ("spat_v_linear_v", ("spat_v_linear_v", 2)), ("spat_q_linear_v", ("spat_q_linear_v", 2)),
          ("spat_att_score", ("spat_att/compute/score", 0)),
          ("gru_wg", _GRU + "gates/kernel"), ("gru_bg", _GRU + "gates/bias"),
          ("gru_wc", _GRU + "candidate/kernel"), ("gru_bc", _GRU + "candidate/bias"),
          ("pooled_linear_l", ("pooled_linear_l", "nh")), ("q_linear_l", ("q_linear_l", "nh")),
          ("wordset_ft", ("wordset_ft", 2)))
_ENWIKI = (("enwiki_map", "enwiki_map/learn"), ("egru_wg", _EGRU + "gates/kernel"), ("egru_bg", _EGRU + "gates/bias"),
           ("egru_wc", _EGRU + "candidate/kernel"), ("egru_bc", _EGRU + "candidate/bias"))
_HEADS = (("joint_fc", ("joint_fc", "nh")), ("classifier", ("classifier", 0)))
_NOC_HEADS = (("joint_v", ("joint_v", "nh")), ("joint_l", ("joint_l", "nh")),
              ("classifier_v", ("classifier_v", 0)), ("classifier_l", ("classifier_l", 0)))
_OPTIONAL = ("wordset_ft",) + tuple(m for m, _ in _ENWIKI)      # without the word-set head / without the enwiki head
PARAM_FIELDS = {_lib.PtParams: _TRUNK + _HEADS,
                _lib.PtExtParams: _TRUNK + _ENWIKI + _HEADS,
                _lib.PtNocParams: _TRUNK + _ENWIKI + _NOC_HEADS,
                _lib.PtAdaptParams: (("ext", _lib.PtExtParams), ("v_adapt", ("v_adapt", 2)))}


PRECISIONS = ("f32", "bf16")      # PretrainEngine(precision=...): "bf16" sets VQA_FLAG_BF16_GEMM
FEATURE_FORMATS = ("f32", "bf16")  # PretrainEngine(features=...): "bf16" sets VQA_FLAG_BF16_FEATURES
ENCODER_FORMATS = ("f32", "bf16")  # PretrainEngine(encoder=...): "bf16" sets VQA_PT_FLAG_BF16_ENCODER


def flat_layout(shapes):
    """Where every variable sits in the flat buffers (pure host arithmetic, no GPU), the twin of fusion.flat_layout:
    train_flat / grad_flat order = [sparse tables | PHASE_SCOPES' groups, by name] (+ 4 tail floats in grad_flat), every
    variable padded to a multiple of 4 floats.  `bounds` (floats): wordset_map [0, b0), L_GloVe (+ enwiki_map) [b0, b1),
    GRUs [b1, b2), heads [b2, b3), rest [b3, n_train).  `buckets` are the slices of grad_flat
    PretrainEngine.backward hands to a bucketed reducer, in the order it starts them."""
    sparse = [k for k in SPARSE_VARS if k in shapes]
    dense = sorted(k for k in shapes if k not in NO_GRAD_VARS and k not in SPARSE_VARS)
    groups = [[k for k in dense if k.startswith(sc)] for sc in PHASE_SCOPES]
    assert sorted(sum(groups, [])) == dense, "a variable outside the phase scopes"
    train_names = sparse + sum(groups, [])
    tab, n_train = carve(train_names, shapes)
    ends, o = [], 0
    for names in ([sparse[0]], sparse[1:], groups[0], groups[1], groups[2]):
        o += carve(names, shapes)[1]
        ends.append(o)
    assert ends[-1] == n_train
    b0, b1, b2, b3 = ends[:4]
    return dict(train_names=train_names, tab=tab, n_train=n_train, bounds=tuple(ends), sparse_floats=b1,
                buckets=[(b2, b3), (b1, b2), (b0, b1), (0, b0), (b3, n_train + 4)])


class PretrainEngine(EngineCore):
    def __init__(self, *, n, R, D, H, W, A, Vq, n_ws, params, device="cuda:0", deterministic=False, ln_shared=None,
                 heads=CFG5_HEADS, n_ctx=None, noc=False, adapt=False, precision="f32", features="f32",
                 encoder="f32"):
        """ln_shared: one LayerNorm per shared fc_layer scope (True) or one per call site (False); None = whatever the
        variable names in `params` say (`.../LayerNorm_1/...` present -> per call site), as for a checkpoint.
        heads: the head set (MODEL_HEADS); with 'ew', n_ctx = the enwiki context vocabulary and every batch carries
        '<kind>_blank_fill/enwiki_context' [B,n,Lc] and '..._len' [B,n].
        noc: the "no composition" model of that head set (NOC_MODEL_HEADS; vqa_pretrain_noc_*).  Its head set (bf, ws)
        equals cfg-5's, so the flag and not the head set selects it.
        adapt: the adapted-memory model (ADAPT_MODEL_HEADS; vqa_pretrain_adapt_*), likewise selected by the flag.
        precision="bf16": opt-in mixed precision -- forward, dW and dx of pooled_linear_l, q_linear_l, joint_fc and the
        classifier (noc: joint_v / joint_l / classifier_v / classifier_l; adapt: also v_adapt) multiply bf16-rounded
        operands with f32 accumulation (ops.gemm_bf16); both encoders, wordset_ft, the box layers and everything that is
        not a GEMM stay f32 (include/vqa_hot.h, VQA_FLAG_BF16_GEMM).  Every head set, noc and adapt.  Parameters,
        gradients, Adam slots, state_dict() and the DP buckets are those of "f32": checkpoints are interchangeable.
        features="bf16" (opt-in, only with precision="bf16"): the region features are bf16 at rest -- bind_tables takes a
        torch.bfloat16 table [N,R,D] (model_vlmap_answer.features_to_bf16 makes one), the gathered image_ft is bf16, a
        batch that carries image_ft itself carries it as torch.bfloat16, and the attention kernels (adapt: v_adapt's
        forward and dW GEMMs) read the 16-bit patterns as they are (VQA_FLAG_BF16_FEATURES).  Half the resident table; the
        step equals, bit for bit, the precision="bf16" step on the same features widened to f32.  Every head set, noc
        and adapt; parameters, checkpoints and DP buckets unchanged.
        encoder="bf16" (opt-in, only with precision="bf16"): both sequence encoders join the routed list -- the
        x-projection, dx, dwx and both dwh on the bf16 GEMM, the per-step recurrence with bf16 operands in its four fused
        step GEMMs (VQA_PT_FLAG_BF16_ENCODER; h, r*h, the backward's d_pre operands and the weights are rounded on their way
        into the matrix unit, the state, the tapes and the gate math stay f32).  Per engine, not process-wide.  Every head
        set, noc and adapt; composes with features="bf16" and seeded dropout; parameters, checkpoints and DP buckets
        unchanged."""
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s, not %r" % (PRECISIONS, precision))
        if features not in FEATURE_FORMATS:
            raise ValueError("features must be one of %s, not %r" % (FEATURE_FORMATS, features))
        if encoder not in ENCODER_FORMATS:
            raise ValueError("encoder must be one of %s, not %r" % (ENCODER_FORMATS, encoder))
        if encoder == "bf16" and precision != "bf16":
            raise ValueError("encoder='bf16' needs precision='bf16' (the flag is valid only on top of the bf16 GEMMs)")
        if features == "bf16" and precision != "bf16":
            raise ValueError("features='bf16' needs precision='bf16' (the f32 products read f32 features)")
        self.precision = precision
        self.features = features
        self.encoder = encoder
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.VqaHotError("PretrainEngine needs a GPU (no CPU fallback)")
        self.heads = tuple(heads)
        self.noc, self.adapt = bool(noc), bool(adapt)
        if self.noc and self.adapt:
            raise ValueError("the reference has no model that is both noc and adapt")
        if self.heads not in (NOC_MODEL_HEADS if self.noc else ADAPT_MODEL_HEADS if self.adapt else MODEL_HEADS).values():
            raise ValueError("unsupported head set %r%s" % (self.heads, " for a noc model" if self.noc else
                                                            " for the adapt model" if self.adapt else ""))
        # vqa_pretrain_ext_* (the cfg-5 head set keeps vqa_pretrain_*); noc / adapt: vqa_pretrain_noc_* / _adapt_* on the
        # ext dims / batch
        self.ext = self.noc or self.adapt or self.heads != CFG5_HEADS
        self._abi = "vqa_pretrain_noc_" if self.noc else "vqa_pretrain_adapt_" if self.adapt else \
            "vqa_pretrain_ext_" if self.ext else "vqa_pretrain_"
        self.n_ctx = int(n_ctx) if "ew" in self.heads else None
        self.report_keys = report_keys(self.heads, self.noc)
        self.device = torch.device(device)
        self.n, self.R, self.D, self.H, self.W, self.A = n, R, D, H, W, A
        self.Vq, self.n_ws, self.deterministic = Vq, n_ws, bool(deterministic)
        self.step_count, self.clip_norm = 0, CLIP_NORM
        self.report, self._micro_report = {}, None
        self.workspace, self.dims = None, None
        self._layout(ln_shared_in(params) if ln_shared is None else bool(ln_shared))
        for k in self.shapes:
            self.params[k].copy_(torch.as_tensor(np.asarray(params[k])).to(torch.float32))

    def _layout(self, ln_shared):
        """Flat parameter / gradient / Adam buffers and the C structs for one of the two LayerNorm variable sets."""
        self.ln_shared = bool(ln_shared)
        self.shapes = variable_shapes(self.Vq, self.n_ws, self.A, self.W, self.D, self.H, self.ln_shared, self.heads,
                                      self.n_ctx, self.noc, self.adapt)
        lay = flat_layout(self.shapes)
        self.train_names, self._tab, self._bounds = lay["train_names"], lay["tab"], lay["bounds"]
        self.sparse_floats = lay["sparse_floats"]
        self._alloc_flat(self._tab, lay["n_train"], self.shapes, self.sparse_floats, self.device)
        self._set_schedule(phase_schedule(BUCKET_PHASES, lay["buckets"]))
        for k in NO_GRAD_VARS:
            self.params[k] = torch.zeros(self.shapes[k], dtype=torch.float32, device=self.device)
        self._p_struct = self._param_struct(self.params)
        self._g_struct = self._param_struct(self.grads)

    def _flags(self):
        return (_lib.FLAG_DETERMINISTIC if self.deterministic else 0) | (_lib.FLAG_SHARED_LN if self.ln_shared else 0) | \
            (_lib.FLAG_BF16_GEMM if self.precision == "bf16" else 0) | \
            (_lib.FLAG_BF16_FEATURES if self.features == "bf16" else 0) | \
            (_lib.PT_FLAG_BF16_ENCODER if self.encoder == "bf16" else 0)

    # ------------------------------------------------------------------ C-ABI plumbing
    def keep_offsets(self, B, step, row_offset=0, global_rows=None):
        """The layout of the dropout stream at `step`, the ONE copy of its arithmetic: {site: (offset, elements per image,
        keep_prob)} for the sites {kind/att, kind/bf_joint, kind/ws_joint} (the cfg-5 region), {kind}/ew_joint (with the
        enwiki head: their own counter range from EW_MASK_COUNTER) and {kind}/{head}_joint_l (noc: the l branch, a third
        range from NOC_L_MASK_COUNTER; the v branch uses the joint sites).  `offset` is the stream position of the site's
        element 0 for THESE B images.  The stream is indexed by the GLOBAL image row: a data-parallel shard of B images
        passes its first global row (row_offset) and the global batch size, and its sites then start at the bits one
        process on the whole batch draws for those rows.  make_keep_masks writes these streams into tensors; with
        dropout=(seed, step) the kernels compute them in place."""
        n, R, H = self.n, self.R, self.H
        Bg = int(global_rows) if global_rows is not None else B
        out, off = {}, step * (2 * (Bg * n * R * H + 2 * Bg * n * 2 * H))
        for k in KINDS:
            for name, per_image, keep in ((k + "/att", n * R * H, KEEP_ATT), (k + "/bf_joint", n * 2 * H, KEEP_JOINT),
                                          (k + "/ws_joint", n * 2 * H, KEEP_JOINT)):
                out[name] = (off + row_offset * per_image, per_image, keep)
                off += Bg * per_image
        per_image = n * 2 * H
        if "ew" in self.heads:
            # their own counter range: the cfg-5 sites above keep their bits for (seed, step, row)
            off = EW_MASK_COUNTER + step * (2 * Bg * per_image)
            for k in KINDS:
                out[k + "/ew_joint"] = (off + row_offset * per_image, per_image, KEEP_JOINT)
                off += Bg * per_image
        if self.noc:
            off = NOC_L_MASK_COUNTER + step * (2 * len(self.heads) * Bg * per_image)
            for h in self.heads:
                for k in KINDS:
                    out["%s/%s_joint_l" % (k, h)] = (off + row_offset * per_image, per_image, KEEP_JOINT)
                    off += Bg * per_image
        return out

    def make_keep_masks(self, B, seed, step, row_offset=0, global_rows=None):
        """reproducible dropout keep-masks for (seed, step): uint8 tensors of the sites of keep_offsets, by site name"""
        return {name: ops.dropout_mask(B * per_image, seed, off, keep, self.device)
                for name, (off, per_image, keep) in self.keep_offsets(B, step, row_offset, global_rows).items()}

    def _keep_struct(self, B, dropout):
        """vqa_pretrain_keep_t of dropout = (seed, step[, row_offset, global_rows]): every site the model has is seeded"""
        seed, step = int(dropout[0]), int(dropout[1])
        row_offset, global_rows = (dropout[2], dropout[3]) if len(dropout) == 4 else (0, None)
        offs = self.keep_offsets(B, step, int(row_offset or 0), global_rows)
        ks = _lib.PtKeep(keep_seed=seed)
        for ki, k in enumerate(KINDS):
            for site in ("att", "bf_joint", "ws_joint", "ew_joint"):
                if k + "/" + site in offs:
                    getattr(ks, site + "_off")[ki] = offs[k + "/" + site][0]
                    ks.seeded |= _lib.PT_KEEP_SITE[site]
            for ti, h in enumerate(("bf", "ws", "ew")):
                if "%s/%s_joint_l" % (k, h) in offs:
                    ks.l_joint_off[ki][ti] = offs["%s/%s_joint_l" % (k, h)][0]
                    ks.seeded |= _lib.PT_KEEP_SITE["l_joint"]
        return ks

    def _param_struct(self, table, struct=None):
        """The C struct `struct` (default: the one this engine's entry points take) filled from the name -> tensor
        `table` by PARAM_FIELDS; an _OPTIONAL member the table lacks stays NULL, any other missing variable raises."""
        struct = struct or {"vqa_pretrain_": _lib.PtParams, "vqa_pretrain_ext_": _lib.PtExtParams,
                            "vqa_pretrain_noc_": _lib.PtNocParams, "vqa_pretrain_adapt_": _lib.PtAdaptParams}[self._abi]
        types = dict(struct._fields_)

        def fc(f, scope, n_ln):
            f.w, f.b = table[scope + "/fc/weights"].data_ptr(), table[scope + "/fc/biases"].data_ptr()
            n_ln = 2 * len(self.heads) if n_ln == "nh" else n_ln
            for i in range(min(n_ln, 1) if self.ln_shared else n_ln):
                f.beta[i] = table[ln_name(scope, i) + "/beta"].data_ptr()
                f.gamma[i] = table[ln_name(scope, i) + "/gamma"].data_ptr()
            return f
        out = struct()
        for member, src in PARAM_FIELDS[struct]:
            if member in _OPTIONAL and (src[0] + "/fc/weights" if isinstance(src, tuple) else src) not in table:
                continue
            if isinstance(src, tuple):
                setattr(out, member, fc(types[member](), *src))
            elif isinstance(src, str):
                setattr(out, member, table[src].data_ptr())
            else:
                setattr(out, member, self._param_struct(table, src))
        return out

    def _dev(self, v, dtype):
        t = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def bind_tables(self, image_features, spatial_features, num_boxes):
        """Keep the feature tables of the dataset ([N,R,D] f32, [N,R,6] f32, [N] i32) in HBM; batches may then carry
        `image_idx` (i64 [B]) instead of image_ft / spatial_ft / num_boxes and the rows are gathered on the device
        (`vqa_gather_features`), the cfg-5 counterpart of SURVEY row a1: no per-step np.take of 151 MB on the host and
        no H2D copy of it.  The reference holds the whole '<split>_vfeat.hdf5' in host RAM (dataset_vlmap.py:67-72).
        features="bf16": image_features is a contiguous torch.bfloat16 device table [N,R,D], never converted here."""
        if self.features == "bf16":
            f = image_features
            if not (torch.is_tensor(f) and f.dtype == torch.bfloat16 and f.is_cuda and f.is_contiguous()
                    and f.dim() == 3 and tuple(f.shape[1:]) == (self.R, self.D)):
                raise ValueError("features='bf16' needs a contiguous torch.bfloat16 device table [N, %d, %d] (got %s %s); "
                                 "model_vlmap_answer.features_to_bf16 converts an f32 array"
                                 % (self.R, self.D, getattr(f, "dtype", type(f)), tuple(getattr(f, "shape", ()))))
        else:
            f = self._dev(image_features, torch.float32)
        assert f.dim() == 3 and f.shape[1] == self.R and f.shape[2] == self.D, f.shape
        self._tables = (f, self._dev(spatial_features, torch.float32), self._dev(np.asarray(num_boxes), torch.int32))
        self._gathered = {}

    def _gather(self, idx):
        """image_ft / spatial_ft / num_boxes of a batch from the bound tables, into buffers owned by the engine"""
        from . import ops
        table, spat, nb = self._tables
        B = int(idx.numel())
        buf = self._gathered.get(B)
        if buf is None:
            buf = self._gathered[B] = {"spatial_ft": torch.empty(B, self.R, spat.shape[2], device=self.device)}
        V, n = (ops.gather_features_bf16 if self.features == "bf16" else ops.gather_features)(table, nb, idx)
        torch.index_select(spat, 0, idx, out=buf["spatial_ft"])
        return V, buf["spatial_ft"], n

    def _batch_struct(self, batch, masks):
        """C view of one batch (device tensors with the keys of vlmap_memft/datasets/dataset_vlmap.py:128-236 that
        the model reads).  Converted tensors are cached on the batch dict, so a batch that is fed again (the input
        pipeline caches its batches) costs no conversion."""
        cache = batch.setdefault("_pt_dev", {}) if isinstance(batch, dict) else {}
        def get(key, dtype):
            if key not in cache:
                cache[key] = self._dev(batch[key], dtype)
            return cache[key]
        keep = [cache, masks]

        def sort_ptrs(key, length):
            """(perm, inv, live_rows) pointers of the rows' length order batch[key] (add_length_sort), or three NULLs;
            uploaded once and cached on the sort dict"""
            srt = batch.get(key)
            if srt is None:
                return None, None, None
            if "_dev" not in srt:
                live = np.ascontiguousarray(srt["live_rows"], dtype=np.int32)
                assert live.shape == (length,) and \
                    len(srt["perm"]) == 2 * int(cache[KINDS[0] + "_blank_fill/blanks_len"].numel())
                srt["_dev"] = (self._dev(np.asarray(srt["perm"]), torch.int32),
                               self._dev(np.asarray(srt["inv"]), torch.int32), live)
            perm, inv, live = srt["_dev"]
            keep.append(srt["_dev"])
            return perm.data_ptr(), inv.data_ptr(), live.ctypes.data
        if "image_idx" in batch and "image_ft" not in batch:
            if getattr(self, "_tables", None) is None:
                raise ValueError("batch carries image_idx but no feature tables are bound (PretrainEngine.bind_tables)")
            V, sp, nb = self._gather(get("image_idx", torch.int64))
            keep.append((V, sp, nb))
            bs = _lib.PtBatch(image_ft=V.data_ptr(), spatial_ft=sp.data_ptr(), num_boxes=nb.data_ptr())
            B = V.shape[0]
        else:
            if self.features == "bf16":      # as the table: bf16 already, never converted here
                ft = batch["image_ft"]
                if not (torch.is_tensor(ft) and ft.dtype == torch.bfloat16 and ft.is_cuda and ft.is_contiguous()
                        and ft.dim() == 3 and tuple(ft.shape[1:]) == (self.R, self.D)):
                    raise ValueError("features='bf16' needs image_ft as a contiguous torch.bfloat16 device tensor "
                                     "[B, %d, %d] (got %s %s); model_vlmap_answer.features_to_bf16 converts an f32 array"
                                     % (self.R, self.D, getattr(ft, "dtype", type(ft)), tuple(getattr(ft, "shape", ()))))
                cache["image_ft"] = ft
            bs = _lib.PtBatch(image_ft=get("image_ft", torch.float32).data_ptr(),
                              spatial_ft=get("spatial_ft", torch.float32).data_ptr(),
                              num_boxes=get("num_boxes", torch.int32).data_ptr())
            B = cache["image_ft"].shape[0]
        L = None
        for ki, k in enumerate(KINDS):
            pre = k + "_blank_fill/"
            kb = bs.kind[ki]
            kb.normal_boxes = get(pre + "normal_boxes", torch.float32).data_ptr()
            for f in ("fills", "blanks", "blanks_len", "wordsets", "num"):
                setattr(kb, f, get(pre + f, torch.int32).data_ptr())
            Lk = int(cache[pre + "blanks"].shape[-1])
            assert L is None or L == Lk, "object / attribute captions must be padded to one length"
            L = Lk
            if masks is not None:
                kb.keep_att = masks[k + "/att"].data_ptr()
                kb.keep_bf_joint = masks[k + "/bf_joint"].data_ptr()
                kb.keep_ws_joint = masks[k + "/ws_joint"].data_ptr()
        # captions in length order: the recurrence skips finished ones
        bs.perm, bs.inv, bs.live_rows = sort_ptrs("blank_fill/sort", L)
        if not self.ext:
            return bs, B, L, keep
        bx = _lib.PtExtBatch(base=bs)
        Lc = None
        for ki, k in enumerate(KINDS if "ew" in self.heads else ()):
            pre = k + "_blank_fill/"
            ck = bx.ctx[ki]
            ck.context = get(pre + "enwiki_context", torch.int32).data_ptr()
            ck.context_len = get(pre + "enwiki_context_len", torch.int32).data_ptr()
            Lk = int(cache[pre + "enwiki_context"].shape[-1])
            assert Lc is None or Lc == Lk, "object / attribute contexts must be padded to one length"
            Lc = Lk
            if masks is not None:
                ck.keep_ew_joint = masks[k + "/ew_joint"].data_ptr()
        bx.ctx_perm, bx.ctx_inv, bx.ctx_live_rows = sort_ptrs("enwiki_context/sort", Lc)      # add_context_sort
        self._Lc = Lc
        if not self.noc:
            return bx, B, L, keep
        bn = _lib.PtNocBatch(base=bx)
        if masks is not None:         # the l branch's keep-masks (make_keep_masks: '<kind>/<head>_joint_l')
            for ki, k in enumerate(KINDS):
                for h in self.heads:
                    setattr(bn.l[ki], "keep_%s_l_joint" % h, masks["%s/%s_joint_l" % (k, h)].data_ptr())
        return bn, B, L, keep

    def tensor(self, name, dtype=torch.float32):
        """Named intermediate of the last forward as a torch view of the workspace (vqa_pretrain_tensor)."""
        off, n = C.c_int64(), C.c_int64()
        fn = getattr(self.lib, self._abi + "tensor")
        _lib.check(fn(C.byref(self.dims), name.encode(), C.byref(off), C.byref(n)), "vqa_pretrain_tensor(%s)" % name)
        return self.workspace[off.value:off.value + 4 * n.value].view(dtype)

    # ------------------------------------------------------------------ forward / backward
    def global_valid_counts(self, batch, group=None):
        """(#valid object entries, #valid attribute entries) of the GLOBAL batch = the denominators of the masked mean
        losses (n_way_classification_loss, :675-706): this shard's counts, SUM-all-reduced over the ranks.  A trainer
        whose ranks slice one global batch can compute the same numbers from the host arrays without a collective."""
        import torch.distributed as dist
        cnt = torch.stack([torch.as_tensor(batch[k + "_blank_fill/num"]).to(torch.int64).clamp(0, self.n).sum()
                           for k in KINDS]).to(torch.float64)
        if dist.is_initialized() and dist.get_world_size(group) > 1:
            if dist.get_backend(group) == "gloo":
                cnt = cnt.cpu()
            else:
                cnt = cnt.to(self.device)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
        return tuple(float(v) for v in cnt.cpu())

    def forward(self, batch, masks, want_dz=True, global_valid=None, dropout=None, row_offset=0, global_rows=None):
        """batch: dict of arrays / tensors (keys of dataset_vlmap's batches; optional 'blank_fill/sort' from
        add_length_sort); masks: uint8 keep-masks keyed '<kind>/att|bf_joint|ws_joint' or None (no dropout);
        global_valid: data parallel only -- (object, attribute) valid-entry counts of the global batch.
        dropout=(seed, step) or (seed, step, row_offset, global_rows): seeded dropout -- the bits of
        make_keep_masks(B, seed, step, row_offset, global_rows), computed inside the attention and LayerNorm kernels that
        consume them (vqa_pretrain_*_ex); no mask tensor exists, and the step is bit for bit the step on those masks.
        Exclusive with masks.  row_offset / global_rows may also be given by keyword."""
        if dropout is not None:
            if masks is not None:
                raise ValueError("masks and dropout=(seed, step) are mutually exclusive")
            if len(dropout) == 2:
                dropout = (dropout[0], dropout[1], row_offset, global_rows)
            elif len(dropout) != 4:
                raise ValueError("dropout is (seed, step) or (seed, step, row_offset, global_rows)")
        bs, B, L, keep = self._batch_struct(batch, masks)
        self._micro_report = None     # fetch_report speaks of THIS batch again (train_micro_steps sets it after its last)
        self._ks = self._keep_struct(B, dropout) if dropout is not None else None
        d = _lib.PtDims(B=B, n=self.n, R=self.R, D=self.D, H=self.H, W=self.W, A=self.A, Vq=self.Vq, n_ws=self.n_ws, L=L,
                        flags=self._flags(), keep_att=KEEP_ATT,
                        keep_joint=KEEP_JOINT)
        if global_valid is not None:
            d.global_valid[0], d.global_valid[1] = float(global_valid[0]), float(global_valid[1])
        if self.ext:
            d = _lib.PtExtDims(base=d, heads=head_mask(self.heads), Lc=self._Lc or 0, n_ctx=self.n_ctx or 0)
        self._ensure_workspace(getattr(self.lib, self._abi + "workspace_bytes"), d,
                               "vqa_pretrain_workspace_bytes rejected the dims")
        self.dims, self._bs, self._keepalive = d, bs, keep
        fwd = getattr(self.lib, self._abi + "forward_ex")
        _lib.check(fwd(C.byref(d), C.byref(self._p_struct), C.byref(bs), C.c_void_p(self.workspace.data_ptr()),
                       self.workspace.numel(), 1 if want_dz else 0, self._stream(),
                       C.byref(self._ks) if self._ks is not None else None), "vqa_pretrain_forward")
        Bn = B * self.n
        zs = ("zv", "zl") if self.noc else ("z",)       # noc: the two branches' logits of every head
        self._tape = {"B": B, "kinds": {
            k: dict({"att": self.tensor(k + "/att").view(Bn, self.R),
                     "pooled": self.tensor(k + "/pooled").view(Bn, self.H if self.adapt else self.D)},
                    **{TASK_NAMES[h]: {z: self.tensor("%s/%s/%s" % (k, h, z)).view(Bn, self.A) for z in zs}
                       for h in self.heads})
            for k in KINDS}}

    def fetch_report(self, reduce=False, group=None):
        """report dict of the reference (13 scalars, 19 with the enwiki heads or a noc model): <kind>_<task>_{loss,acc,
        top_5_acc} (noc SPLIT heads: <kind>_<task>_{v,l}_{...}), total_loss.  reduce: data parallel -- every scalar is a sum over the shard's rows already divided by the GLOBAL
        valid count (forward(global_valid=...)), so a SUM all-reduce gives what one process on the whole batch reports."""
        import torch.distributed as dist
        nk = len(self.report_keys)
        mr = getattr(self, "_micro_report", None)
        # after train_micro_steps: the micro-batches' scalars, summed -- each was divided by the step's global valid counts
        r = self.tensor("report")[:nk] if mr is None else mr["stats"]
        group = group if group is not None or mr is None else mr["group"]
        reduce = reduce or (mr is not None and mr["dp"])
        if reduce and dist.is_initialized() and dist.get_world_size(group) > 1:
            r = r.cpu() if dist.get_backend(group) == "gloo" else r.clone()
            dist.all_reduce(r, op=dist.ReduceOp.SUM, group=group)
        r = r.cpu().numpy()
        self.report = {self.report_key(i): float(r[i]) for i in range(nk)}
        return self.report

    def report_key(self, i):
        """name of report scalar i (vqa_pretrain_report_key / vqa_pretrain_ext_report_key)"""
        fn = getattr(self.lib, self._abi + "report_key")
        return (fn(head_mask(self.heads), i) if self.ext else fn(i)).decode()      # cfg-5's takes no head set

    def _backward_phases(self, phases):
        tail = self.grad_flat[self.n_train:]
        fn = getattr(self.lib, self._abi + "backward_phases_ex")      # the forward's keep struct: the bits are regenerated
        _lib.check(fn(
            C.byref(self.dims), C.byref(self._p_struct), C.byref(self._g_struct), C.byref(self._bs),
            C.c_void_p(self.workspace.data_ptr()), self.workspace.numel(), C.c_void_p(tail.data_ptr()), phases,
            self._stream(), C.byref(self._ks) if self._ks is not None else None), "vqa_pretrain_backward_phases")

    def train_step(self, batch, masks, lr, allreduce=None, global_valid=None, dropout=None, row_offset=0, global_rows=None):
        """forward -> backward -> (gradient all-reduce) -> clip + Adam.  Data parallel: `allreduce` is a
        dp.BucketedAllReduce (overlapped with the backward phases) or any callable on grad_flat; pass the global
        valid counts so that every shard divides by the global denominators and a SUM reduce gives the gradient of
        the global-batch losses; all ranks then apply the identical update.  dropout: as for forward."""
        self.forward(batch, masks, global_valid=global_valid, dropout=dropout, row_offset=row_offset, global_rows=global_rows)
        self._backward_and_step(lr, allreduce)

    # ------------------------------------------------------------------ micro-batched step (EngineCore.train_micro_steps)
    # micro[i] = {"batch": ..., "masks": keep-masks of make_keep_masks(B_i, seed, step, row_offset_i, G) | None,
    #             or "dropout": (seed, step)}; train_micro_steps(..., global_valid=(obj, attr)) as for train_step
    def _micro_rows(self, m):
        b = m["batch"]
        return int(len(b["image_idx"] if "image_idx" in b and "image_ft" not in b else b["image_ft"]))

    def _micro_open(self, micro, G, dp, allreduce, global_valid=None):
        """The denominators of the masked mean losses are the GLOBAL batch's valid-entry counts: the pre-training step's
        1/G.  One micro-batch keeps what train_step does with None (the batch's own counts, taken on the device); more
        than one needs them summed over the micro-batches (and, data parallel, over the ranks) before the first runs.
        Summing them HERE reads every micro-batch's `num` back (a host synchronisation per micro-batch when the batches are
        device tensors): a caller that has the host arrays passes global_valid, as the trainer's model does."""
        if global_valid is None and (len(micro) > 1 or dp):
            import torch.distributed as dist
            group = getattr(allreduce, "group", None)
            cnt = torch.zeros(2, dtype=torch.float64)
            for m in micro:
                cnt += torch.stack([torch.as_tensor(m["batch"][k + "_blank_fill/num"]).to(torch.int64).clamp(0, self.n).sum()
                                    for k in KINDS]).to(torch.float64).cpu()
            if dp and dist.is_initialized() and dist.get_world_size(group) > 1:
                if dist.get_backend(group) != "gloo":
                    cnt = cnt.to(self.device)
                dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
            global_valid = tuple(float(v) for v in cnt.cpu())
        return {"global_valid": global_valid}

    def _micro_forward(self, m, row_offset, G, ctx):
        if "dropout" in m and m["dropout"] is not None and len(m["dropout"]) != 2:
            raise ValueError("a micro-batch's dropout is (seed, step): train_micro_steps places its rows in the global batch")
        self.forward(m["batch"], m.get("masks"), global_valid=ctx["global_valid"], dropout=m.get("dropout"),
                     row_offset=row_offset, global_rows=G)

    def _micro_stats(self):
        """this micro-batch's report scalars: sums over its rows already divided by the global valid counts, so they add"""
        return self.tensor("report")[:len(self.report_keys)].clone()

    def _micro_close(self, ctx):
        pass

    def load_state_dict(self, sd, strict=True):
        """Restores parameters, Adam moments and the step count (beta powers), so a resumed run continues the
        optimiser trajectory of an uninterrupted one.  The LayerNorm variable set follows the NAMES in the checkpoint:
        `<scope>/LayerNorm_1/...` present -> one LayerNorm per call site, absent -> one per shared scope; an engine
        built for the other set is laid out again before loading.  strict: a model variable missing from the
        checkpoint raises (a silently skipped name would resume from the initial weights)."""
        model_keys = [k for k in sd if k != "global_step" and not k.endswith(("/Adam", "/Adam_1"))]
        shared = ln_shared_in(model_keys)
        if shared != self.ln_shared:
            self._layout(shared)
            self.workspace, self.dims = None, None
        missing = [k for k in self.shapes if k not in sd]
        if missing and strict:
            raise KeyError("checkpoint lacks %d model variables, e.g. %s" % (len(missing), ", ".join(sorted(missing)[:4])))
        for k in self.shapes:
            if k in sd:
                self.params[k].copy_(torch.as_tensor(sd[k]).to(torch.float32))
        self._load_optimizer_state(sd)
        return missing


def export_word_weights(state_dict, vocab, answer_dict, save_dir):
    """vlmap_memft/export_word_weights.py:35-82: the bridge from pre-training to the VQA model
    (modules.WordWeightAnswer reads class_weights / class_biases by answer string).  Writes weights.hdf5 with the
    reference's five datasets (hdf5_io, no h5py) and vocab.pkl / answer_dict.pkl like the reference."""
    import os
    import pickle
    from . import hdf5_io
    if os.path.exists(save_dir):
        raise ValueError("Do not overwrite: {}".format(save_dir))
    os.makedirs(save_dir)
    g = lambda k: np.asarray(state_dict[k].cpu() if torch.is_tensor(state_dict[k]) else state_dict[k])
    hdf5_io.write(os.path.join(save_dir, "weights.hdf5"),
                  {"v_word": g("V_GloVe/embed_map"), "l_word": g("L_GloVe/embed_map"),
                   "l_answer_word": g("LearnAnswerGloVe/embed_map"), "class_weights": g("classifier/fc/weights"),
                   "class_biases": g("classifier/fc/biases")})
    with open(os.path.join(save_dir, "vocab.pkl"), "wb") as f:
        pickle.dump(vocab, f)
    with open(os.path.join(save_dir, "answer_dict.pkl"), "wb") as f:
        pickle.dump(answer_dict, f)
    return save_dir


def export_noc_word_weights(state_dict, vocab, answer_dict, save_dir):
    """vlmap_memft/export_noc_word_weights.py:35-95 for a checkpoint of a noc model (what vlmap_answer_noc reads through
    --vlmap_word_weight_dir): weights.hdf5 with v_word, l_word, l_answer_word and the two heads' v_class_* / l_class_*
    (export_noc_word_weights.DATASETS), vocab.pkl and answer_dict.pkl."""
    import os
    import pickle
    from . import hdf5_io
    from .export_noc_word_weights import DATASETS
    if os.path.exists(save_dir):
        raise ValueError("Do not overwrite: {}".format(save_dir))
    missing = [name for _, name in DATASETS if name not in state_dict]
    if missing:
        raise KeyError("not a noc checkpoint: no %s" % ", ".join(missing))
    os.makedirs(save_dir)
    g = lambda k: np.asarray(state_dict[k].cpu() if torch.is_tensor(state_dict[k]) else state_dict[k])
    hdf5_io.write(os.path.join(save_dir, "weights.hdf5"), {ds: g(name) for ds, name in DATASETS})
    with open(os.path.join(save_dir, "vocab.pkl"), "wb") as f:
        pickle.dump(vocab, f)
    with open(os.path.join(save_dir, "answer_dict.pkl"), "wb") as f:
        pickle.dump(answer_dict, f)
    return save_dir
