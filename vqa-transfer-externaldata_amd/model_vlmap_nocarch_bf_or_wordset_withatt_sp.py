"""Model class of vlmap_memft/model_vlmap_nocarch_bf_or_wordset_withatt_sp.py, a byte-identical copy of
model_vlmap_noc_bf_or_wordset_withatt_sp.py registered under its own name."""
from __future__ import annotations

from .model_vlmap_noc_bf_or_wordset_withatt_sp import Model as _NocModel


class Model(_NocModel):
    MODEL_TYPE = "vlmap_nocarch_bf_or_wordset_withatt_sp"
