"""Model class of vlmap_memft/model_vlmap_noc_bf_or_enwiki_withatt_sp.py: the "no composition" fusion of
model_vlmap_noc_bf_or_wordset_withatt_sp with the enwiki-context head in place of the word-set head (blank fill SUM,
enwiki SPLIT: <kind>_enwiki_v_* and _l_* report keys; 19 scalars).  wordset_map exists and receives no gradient; the
word sets come from 'wordset_dict5.pkl'.  Batches carry {obj,attr}_blank_fill/enwiki_context[_len]."""
from __future__ import annotations

from .model_vlmap_noc_bf_or_wordset_withatt_sp import Model as _NocModel


class Model(_NocModel):
    MODEL_TYPE = "vlmap_noc_bf_or_enwiki_withatt_sp"
