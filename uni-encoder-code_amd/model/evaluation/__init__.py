"""`from model.evaluation import ...` (train_net.py:43-48) resolves here: the evaluation loop and evaluator names of uenc.evaluation."""
from uenc.evaluation import (COCOEvaluator, COCOPanopticEvaluator, CityscapesDepthEvaluator, CityscapesInstanceEvaluator,  # noqa: F401
                             DatasetEvaluator, DatasetEvaluators, InstanceSegEvaluator, KITTIDepthEvaluator, PanopticEvaluator,
                             SemSegEvaluator, build_evaluator, inference_context, inference_on_dataset, print_csv_format)
