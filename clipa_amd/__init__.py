"""clipa_amd - MI355X-native compute engine for the CLIPA / open_clip training step.

Public surface mirrors `open_clip` (clipa_torch/open_clip/__init__.py) for the ViT-CLIP hot path:
create_model, create_model_and_transforms, create_loss, CLIP, ClipLoss, DistillClipLoss, SigLipLoss,
convert_weights_to_lp,
get_cast_dtype, list_models, add_model_config; and the trainer's validation (training/train.py: evaluate,
get_clip_metrics), multi-caption image-text retrieval (`image_text_retrieval`, `evaluate_retrieval`) and the few-shot
linear probe (`fewshot_lsr`, `fewshot_metrics`, `evaluate_fewshot`) and fused fp32 zero-shot classification
(`build_classifier`, `class_mean_embeddings`, `zero_shot_ranks`, `zero_shot_counts`, `zero_shot_metrics`, `evaluate_zero_shot`)
and top-k similarity search (`topk_similarity`, `classify_topk`, `zero_shot_predict`, `retrieve_topk`, `knn_classify`,
`knn_metrics`) and the logistic-regression linear probe of Radford et al. 2021 (`fit_logreg`, `logreg_objective`,
`sweep_l2`, `evaluate_linear_probe`, and `linear_probe.linear_probe` in the module of that name); the device-side input
pipeline (`DeviceAugment`, `DeviceEvalTransform`, `DevicePrefetcher`) over batches of images of mixed sizes (`RaggedImages`,
`pack_images`, `ragged_collate`, `eval_geometry`); and supervised fine-tuning of the image tower (`ImageClassifier`,
`create_classifier`, `SoftTargetCrossEntropy`, `soft_target_cross_entropy`, `DeviceMixCut`, `sample_mixcut`,
`evaluate_classification`).
"""
from .configs import add_model_config, get_model_config, list_models
from .factory import (create_loss, create_model, create_model_and_transforms, get_cast_dtype, load_checkpoint)
from .loss import ClipLoss, DistillClipLoss, SigLipLoss
from .model import (CLIP, CLIPTextCfg, CLIPVisionCfg, OPENAI_DATASET_MEAN, OPENAI_DATASET_STD, convert_weights_to_lp,
                    get_2d_sincos_pos_embed, resize_pos_embed, resize_text_pos_embed)

from .data import (DeviceAugment, DeviceEvalTransform, DevicePrefetcher, RaggedImages, eval_geometry, pack_images,
                   ragged_collate)
from . import fewshot
from .evaluate import evaluate, get_clip_metrics, metrics_from_ranks
from .fewshot import evaluate_fewshot, fewshot_lsr, fewshot_metrics
from . import linear_probe      # the module: its `linear_probe` function is clipa_amd.linear_probe.linear_probe
from .linear_probe import evaluate_linear_probe, fit_logreg, logreg_objective, sweep_l2
from .retrieval_eval import evaluate_retrieval, image_text_retrieval
from .transform import AugmentationCfg, image_transform
from .zero import ShardedAdamW
from . import zero_shot
from .zero_shot import (build_classifier, class_mean_embeddings, evaluate_zero_shot, zero_shot_counts, zero_shot_metrics,
                        zero_shot_ranks)
from . import search
from .search import classify_topk, knn_classify, knn_metrics, retrieve_topk, topk_similarity, zero_shot_predict
from . import finetune
from .finetune import (DeviceMixCut, ImageClassifier, SoftTargetCrossEntropy, evaluate_classification, sample_mixcut,
                       soft_target_cross_entropy)
from .factory import create_classifier

__version__ = "0.4.0"
