"""Model class of vlmap_memft/model_vlmap_bf_enwiki_withatt_sp.py (run.py:104-105): blank-fill and enwiki-context heads,
no word-set head (:83-84) -- wordset_map exists and receives no gradient, wordset_ft does not exist; 13 report
scalars.  Otherwise as model_vlmap_bf_or_wordset_enwiki_withatt_sp."""
from __future__ import annotations

from .model_vlmap_bf_or_wordset_withatt_sp import Model as _Cfg5Model


class Model(_Cfg5Model):
    MODEL_TYPE = "vlmap_bf_enwiki_withatt_sp"
    WS_DICT_FILE = "wordset_dict5.pkl"
