"""Model class of vlmap_memft/model_vlmap_noc_bf_or_wordset_withatt_sp.py, the "no composition" ablation whose checkpoint
feeds vlmap_answer_noc (run_blank_fill_enwiki.py:104-110, 214-239): the cfg-5 model with, per head, the two branches
joint_v -> classifier_v on v_linear_l and joint_l -> classifier_l on l_linear_l instead of joint_fc(v_linear_l * l_linear_l)
-> classifier.  The blank-fill heads' loss is the CE of v_logit + l_logit, the word-set heads have one CE per branch
(<kind>_wordset_v_* and _l_* report keys; 19 scalars).  The word sets come from 'wordset_dict5.pkl' (:34), so
--expand_depth has no effect."""
from __future__ import annotations

from .model_vlmap_bf_or_wordset_withatt_sp import Model as _Cfg5Model


class Model(_Cfg5Model):
    MODEL_TYPE = "vlmap_noc_bf_or_wordset_withatt_sp"
    WS_DICT_FILE = "wordset_dict5.pkl"
    NOC = True
