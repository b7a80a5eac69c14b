"""devias_amd: MI355X-native (gfx950 HIP) implementation of the DEVIAS slot-ViT training step.

Importing the package is cheap and GPU-free; the HIP library is loaded on first kernel use and its absence is an
error (there is no CPU or eager-PyTorch fallback for the hot path)."""
__version__ = "0.1.0"

__all__ = ["create_model", "VisionTransformer", "TrainLoss", "train_class_batch", "ModelEma", "disentangle_vit_base_patch16_224", "MultiTaskTrainLoss", "Mixup", "SoftTargetCrossEntropy", "ClipIngest", "IngestLoader", "RandAugment"]


def __getattr__(name):
    if name in ("create_model", "VisionTransformer", "slot_vit_base_patch16_224", "slot_vit_small_patch16_224",
                "slot_vit_large_patch16_224"):
        from . import modeling_slot
        if name == "create_model":
            from . import modeling_slot_fusion  # noqa: F401  (registers the downstream factories: create_model("slot_fusion_vit_base_patch16_224", ...))
            from . import modeling_finetune  # noqa: F401  (registers the plain video ViT: create_model("vit_base_patch16_224", use_mean_pooling=..., ...))
            from . import modeling_multi_task  # noqa: F401  (registers the two-token multi-task baseline: create_model("disentangle_vit_base_patch16_224", ...))
        return getattr(modeling_slot, name)
    if name in ("slot_fusion_vit_base_patch16_224", "slot_fusion_vit_small_patch16_224", "slot_fusion_vit_large_patch16_224"):
        from . import modeling_slot_fusion
        return getattr(modeling_slot_fusion, name)
    if name == "disentangle_vit_base_patch16_224":
        from . import modeling_multi_task
        return modeling_multi_task.disentangle_vit_base_patch16_224
    if name == "MultiTaskTrainLoss":           # the baseline's TrainLoss (its engine: devias_amd.engine_for_multi_task)
        from .multi_task_loss import TrainLoss
        return TrainLoss
    if name == "TrainLoss":
        from .train_loss import TrainLoss
        return TrainLoss
    if name == "train_class_batch":
        from .engine_for_slot import train_class_batch
        return train_class_batch
    if name == "Mixup":                        # mixup / cutmix on the device (the engines' mixup_fn)
        from .mixup import Mixup
        return Mixup
    if name == "SoftTargetCrossEntropy":       # the criterion of a mixed batch
        from .losses import SoftTargetCrossEntropy
        return SoftTargetCrossEntropy
    if name in ("ClipIngest", "IngestLoader"):  # uint8 frames to the normalised, cropped, resized clip on the device; the loader wrapper that feeds the engines
        from . import ingest
        return getattr(ingest, name)
    if name == "RandAugment":                   # the recipe's RandAugment on the staged uint8 frames, before the ingest
        from .randaug import RandAugment
        return RandAugment
    if name == "ModelEma":
        from .ema import ModelEma
        return ModelEma
    raise AttributeError(name)
