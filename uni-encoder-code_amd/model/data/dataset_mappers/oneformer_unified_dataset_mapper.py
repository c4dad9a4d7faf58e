"""`from model.data.dataset_mappers.oneformer_unified_dataset_mapper import OneFormerUnifiedDatasetMapper` (reference model/__init__.py:8)."""
from uenc.train_data import OneFormerUnifiedDatasetMapper  # noqa: F401

__all__ = ["OneFormerUnifiedDatasetMapper"]
