"""dpvo_amd -- MI355X-native (gfx950) DPVO per-frame update hot path.

Drop-in replacements for cuteboyqq/DPVO's native surface:

  cuda_corr          A-CORR / A-PATCH (+ backward)   -> dpvo_amd.altcorr
  cuda_ba            F-BA / F-REPROJ / F-NBR          -> dpvo_amd.fastba
  lietorch_backends  L-SE3 (SO3 / SE3)                -> dpvo_amd.lietorch
  (net.py Update)    the update operator              -> dpvo_amd.net.Update
  (net.py Patchifier, extractor.py BasicEncoder4)     -> dpvo_amd.Patchifier,
                     the feature encoders and gathers    dpvo_amd.BasicEncoder4
  (dpvo.py __call__ head, terminate / get_pose)      -> dpvo_amd.frontend
  (dpvo.py DPVO, config.py, net.py VONet)            -> dpvo_amd.DPVO,
                     the tracker class                   default_config, VONet
  (net.py VONet.forward, train.py loss and step)      -> dpvo_amd.VONet.forward,
                     the training step                   dpvo_amd.training
  (stream.py image_stream / video_stream)             -> dpvo_amd.stream
  (evaluate_*.py: evo's association, alignment, ATE)  -> dpvo_amd.evaluation
  (data_readers/: frame graph, augmentation, TartanAir) -> dpvo_amd.data_readers

Importing the package puts the in-tree native build on sys.path, so code
written against the reference (`import cuda_corr`) runs the HIP kernels.
"""
from ._native import EXT_NAMES, NATIVE_DIR, c_abi, load_extension  # noqa: F401

__version__ = "0.1.0"

__all__ = ["altcorr", "fastba", "lietorch", "net", "extractor", "projective_ops", "frontend", "load_extension",
           "c_abi", "BasicEncoder4", "Patchifier", "tracker", "DPVO", "default_config", "VONet", "training",
           "CorrBlock", "training_schedule", "flow_loss", "pose_loss", "sequence_loss", "train_step",
           "stream", "evaluation", "read_calib", "prepare_frame", "ImageStream", "ate", "ATEResult", "read_tum",
           "write_tum", "data_readers", "frame_distance_matrix", "build_frame_graph", "FrameGraph",
           "sample_sequence", "AugmentParams", "RGBDAugmentor", "normalize_depth", "RGBDDataset",
           "TartanAir"]


def __getattr__(name):  # the classes, without importing torch.nn at package import
    if name in ("DPVO", "default_config"):
        from . import dpvo

        return getattr(dpvo, name)
    if name in ("VONet", "CorrBlock", "training_schedule"):
        from . import net

        return getattr(net, name)
    if name in ("flow_loss", "pose_loss", "sequence_loss", "train_step"):
        from . import training

        return getattr(training, name)
    if name in ("read_calib", "prepare_frame", "ImageStream"):
        from . import stream

        return getattr(stream, name)
    if name in ("ate", "ATEResult", "read_tum", "write_tum"):
        from . import evaluation

        return getattr(evaluation, name)
    if name in ("frame_distance_matrix", "build_frame_graph", "FrameGraph", "sample_sequence",
                "AugmentParams", "RGBDAugmentor", "normalize_depth", "RGBDDataset", "TartanAir"):
        from . import data_readers

        return getattr(data_readers, name)
    if name == "BasicEncoder4":
        from .extractor import BasicEncoder4

        return BasicEncoder4
    if name == "Patchifier":
        from .net import Patchifier

        return Patchifier
    raise AttributeError(f"module 'dpvo_amd' has no attribute {name!r}")
