"""pyskani_amd — MI355X-native drop-in for pyskani's Database.sketch()/query() hot path.

Mirrors the public names of `pyskani` (src/pyskani/__init__.py:2-16 of the reference).
"""
from .database import Context, Database, Dereplication, Forest, Hit, IntervalHit, Model, Sketch, cluster_records, default_context, forest_records, triangle_matrix

__version__ = "0.1.0"
__author__ = "pyskani_amd authors"
SKANI_VERSION = "0.3.0 (restated; see oracle/README.md)"
__all__ = ["Database", "Hit", "IntervalHit", "Sketch", "Model", "Context", "default_context", "triangle_matrix", "cluster_records", "Dereplication", "forest_records", "Forest", "SKANI_VERSION"]
