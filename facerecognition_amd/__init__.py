"""facerecognition_amd — MI355X-native face-embedding extraction + gallery match.

Drop-in for the hot path of sin0235/FaceRecognition (inference/extract_embeddings.py +
inference/recognition_engine.py + inference/database_builder.py): the Python API keeps the
reference's names and behaviour, the compute runs in the C-ABI HIP library libfrhip.so
(include/frhip.h).  See DESIGN.md.
"""
from .weights import ARCHS, INPUT_SIZE  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):  # lazy: importing the package must not initialise the GPU
    if name == "FRModel":
        from .model import FRModel
        return FRModel
    if name == "DeviceGallery":
        from .gallery import DeviceGallery
        return DeviceGallery
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    if name in _EXPLAIN:
        from . import explainability
        return getattr(explainability, name)
    if name in _LBPH:
        from . import lbph
        return getattr(lbph, name)
    if name == "TSNE":
        from .tsne import TSNE
        return TSNE
    if name in _ARCMARGIN:
        from . import arcmargin
        return getattr(arcmargin, name)
    if name in _TRIPLET:
        from . import triplet
        return getattr(triplet, name)
    if name in _VERIFICATION:
        from . import verification
        return getattr(verification, name)
    if name in _HEAD:
        from . import head
        return getattr(head, name)
    if name in _BACKBONE_TRAIN:
        from . import backbone_train
        return getattr(backbone_train, name)
    if name in _AUGMENT:
        from . import augment
        return getattr(augment, name)
    if name in _OPTIM:
        from . import optim
        return getattr(optim, name)
    if name in _DETECT:
        from . import face_detector
        return getattr(face_detector, name)
    if name == "RecognitionEngine":
        from .recognition_engine import RecognitionEngine
        return RecognitionEngine
    if name in _TRAINER:
        from . import trainer
        return getattr(trainer, name)
    raise AttributeError(name)


_DETECT = ("FaceDetector", "DeviceMTCNN", "detect_face", "synth_mtcnn_state", "load_mtcnn_state")
_OPTIM = ("SGD", "Adam", "AdamW")
_TRAINER = ("ArcFaceTrainer", "EarlyStopping")
_AUGMENT = ("get_train_transforms", "get_val_transforms", "facenet_train_transforms", "DeviceTransform", "mixup_data")
_HEAD = ("EmbeddingHead",)
_BACKBONE_TRAIN = ("Bottleneck", "ResNet50Layer4")
_VERIFICATION = ("verify_pairs", "compute_verification_accuracy", "verification_report")
_TRIPLET = ("TripletLoss", "mine_triplets", "mine_semi_hard_triplets", "mine_batch_hard_triplets", "triplet_loss",
            "online_triplet_loss", "compute_triplet_metrics")
_ARCMARGIN =("ArcMarginProduct", "arcface_loss", "arcface_logits", "class_accuracy")
_EXPLAIN = ("ExplainabilityEngine", "FaceNetExplainabilityEngine", "generate_heatmap", "overlay_heatmap",
            "explain_prediction", "cam_closed_form")
_LBPH = ("LBPHFaceRecognizer", "LBPHFaceRecognizer_create", "train_lbph_model", "recognize_face",
         "find_optimal_threshold", "create_label_map_from_directory", "load_faces_and_labels",
         "train_lbph_from_directory")
_EVALUATE = ("compute_metrics", "threshold_sweep", "roc_analysis", "generate_report", "evaluate_recognition_engine",
             "closed_set_report", "evaluate_closed_set")
