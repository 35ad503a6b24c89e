"""mvsformer_amd — MI355X-native (gfx950) plane-sweep cost-volume path of MVSFormer.

Hand-written HIP kernels behind a C ABI (``include/mvs_hip.h`` -> ``libmvs_hip.so``) re-exposed with the
reference's own Python interface: ``StageNet`` (alias ``DepthNet``), ``CostRegNet``, ``CostRegNet3D``,
``homo_warping_3D_with_mask`` (alias ``homo_warping``), ``depth_regression``, the inverse- and linear-depth schedulers, the depth metrics of ``utils.py``
(``Thres_metrics``, ``AbsDepthError_metrics``, ``metrics.DeviceAverageMeter``, ``metrics.valid_epoch``), the point-cloud scores
(``cloud_eval.evaluate``, ``nn_distance``, ``voxel_downsample``, ``greedy_thin``), and
``install()`` to rebind them inside an unmodified reference checkout.  ``synth`` (pure torch) builds the
synthetic DTU-shaped inputs used by the tests and ``bench.py``.

Importing the package does not load the library; the first op call does and fails loudly if it is missing.
"""
from . import synth  # noqa: F401

__all__ = ["synth", "StageNet", "DepthNet", "CostRegNet", "CostRegNet3D", "CascadeMVS", "homo_warping_3D_with_mask",
           "homo_warping_3D", "homo_warping", "depth_regression", "conf_regression", "init_inverse_range",
           "schedule_inverse_range", "init_range", "schedule_range", "install", "fusion", "FPNDecoder", "FPNDecoderV2", "FPNEncoder", "vit_small", "VisionTransformer",
           "VITDecoderStage4Single", "VITDecoderStage4", "VITDecoderStage4NoAtt", "DINOMVSNet", "SceneFusion", "fuse_scan", "scene", "SceneInference",
           "metrics", "Thres_metrics", "AbsDepthError_metrics", "depth_metrics", "DeviceAverageMeter", "valid_epoch",
           "cloud_eval", "nn_distance", "voxel_downsample", "greedy_thin", "evaluate_cloud", "icp", "evaluate_tt",
           "scene_prep", "prepare_scene"]


def __getattr__(name):
    if name in ("StageNet", "DepthNet"):
        from . import stagenet
        return getattr(stagenet, name)
    if name in ("CostRegNet", "CostRegNet3D", "Conv3d", "Deconv3d", "ConvBnReLU", "depth_regression", "conf_regression",
                "init_inverse_range", "schedule_inverse_range", "init_range", "schedule_range"):
        from . import module
        return getattr(module, name)
    if name in ("homo_warping_3D_with_mask", "homo_warping_3D", "homo_warping", "diff_homo_warping_3D_with_mask"):
        from . import warping
        return getattr(warping, name)
    if name in ("CascadeMVS", "randomize_bn_"):
        from . import cascade
        return getattr(cascade, name)
    if name in ("FPNDecoder", "FPNDecoderV2", "FPNEncoder"):
        from . import fpn
        return getattr(fpn, name)
    if name in ("vit_small", "VisionTransformer", "VITDecoderStage4Single", "VITDecoderStage4", "VITDecoderStage4NoAtt"):
        from . import vit
        return getattr(vit, name)
    if name == "DINOMVSNet":
        from . import mvsformer_model
        return mvsformer_model.DINOMVSNet
    if name == "fusion":
        import importlib
        return importlib.import_module(".fusion", __name__)
    if name in ("SceneFusion", "fuse_scan"):
        from . import fusion
        return getattr(fusion, name)
    if name == "scene":
        import importlib
        return importlib.import_module(".scene", __name__)
    if name == "SceneInference":
        from . import scene
        return scene.SceneInference
    if name == "metrics":
        import importlib
        return importlib.import_module(".metrics", __name__)
    if name in ("Thres_metrics", "AbsDepthError_metrics", "depth_metrics", "DeviceAverageMeter", "valid_epoch"):
        from . import metrics
        return getattr(metrics, name)
    if name == "cloud_eval":
        import importlib
        return importlib.import_module(".cloud_eval", __name__)
    if name in ("nn_distance", "voxel_downsample", "greedy_thin", "icp", "evaluate_tt"):
        from . import cloud_eval
        return getattr(cloud_eval, name)
    if name == "evaluate_cloud":
        from . import cloud_eval
        return cloud_eval.evaluate
    if name == "scene_prep":
        import importlib
        return importlib.import_module(".scene_prep", __name__)
    if name == "prepare_scene":
        from . import scene_prep
        return scene_prep.prepare_scene
    if name == "install":
        from .install import install
        return install
    raise AttributeError(name)
