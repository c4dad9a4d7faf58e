"""`from model.data.build import *` (train_net.py:64): reference model/data/build.py exports build_detection_test_loader; the training
loader is Detectron2's `build_detection_train_loader` (tools/trainers/trainer.py:263), restated in uenc.train_data."""
from uenc.data import build_detection_test_loader  # noqa: F401
from uenc.train_data import build_detection_train_loader  # noqa: F401

__all__ = ["build_detection_test_loader", "build_detection_train_loader"]
