"""`from model.data.dataset_mappers.oneformer_multi_pass_cityscapes_mapper import OneFormerUnifiedMultiPassCityscapesMapper`
(reference model/__init__.py:14)."""
from uenc.train_data import OneFormerUnifiedMultiPassCityscapesMapper  # noqa: F401

__all__ = ["OneFormerUnifiedMultiPassCityscapesMapper"]
