"""Model class of vlmap_memft/model_vlmap_bf_or_wordset_enwiki_withatt_sp.py, the pre-training model of the paper's
pipeline (run.py:104-105): the cfg-5 model plus an enwiki-context head per category (:519-624) -- 19 report scalars.
config additionally carries enwiki_preprocessing (or an in-memory enwiki_dict); the word sets come from
'wordset_dict5.pkl'.  Batches carry {obj,attr}_blank_fill/enwiki_context[_len] (dataset_vlmap.Dataset with enwiki)."""
from __future__ import annotations

from .model_vlmap_bf_or_wordset_withatt_sp import Model as _Cfg5Model


class Model(_Cfg5Model):
    MODEL_TYPE = "vlmap_bf_or_wordset_enwiki_withatt_sp"
    WS_DICT_FILE = "wordset_dict5.pkl"
