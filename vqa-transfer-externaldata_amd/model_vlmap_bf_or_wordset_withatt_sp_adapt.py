"""Model class of vlmap_memft/model_vlmap_bf_or_wordset_withatt_sp_adapt.py (vlmap_memft/trainer.py:58-59), the
pre-training model whose checkpoint vlmap_answer_adapt starts from: the cfg-5 model with
`v_adapt = fc_layer(V_ft, 1024, LayerNorm, ReLU, scope='v_adapt')` (:346-350, :442-446; the LayerNorm runs over the whole
[36, 1024] block of an image) between the region features and `attention_pooling(v_adapt, att_score)` (:365-367,
:461-463).  The pooled vector is 1024-wide, so `pooled_linear_l/fc/weights` is [1024, 1024], the shape
vqa/model_vlmap_answer_adapt.py:73-82 transfers together with q_linear_l and joint_fc.  13-scalar report as cfg-5.  The
word sets come from 'wordset_dict5.pkl' (:34), so --expand_depth has no effect."""
from __future__ import annotations

from .model_vlmap_bf_or_wordset_withatt_sp import Model as _Cfg5Model


class Model(_Cfg5Model):
    MODEL_TYPE = "vlmap_bf_or_wordset_withatt_sp_adapt"
    WS_DICT_FILE = "wordset_dict5.pkl"
    ADAPT = True
