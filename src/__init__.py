"""Import-path compatibility: the reference's experiments do ``from src.diffelastic.diff_model import ...``,
``from src.ddsp.oscillator import ...``, ``from src.lobpcg import ...`` (reference
experiments/material_sync_train.py:14-20).  These modules only re-export ``diffsound_amd``."""

# A namespace that extends over every ``src`` directory on sys.path (this tree first), so the reference's modules this
# project does not provide (src.dmtet.render, src.dmtet.geometry.sdf, ...) still import when its tree is second on
# PYTHONPATH.
import pkgutil

__path__ = pkgutil.extend_path(__path__, __name__)
