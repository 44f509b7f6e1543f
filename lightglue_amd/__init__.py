"""lightglue_amd — MI355X-native (gfx950) LightGlue matcher forward path.

Drop-in for the hot path of cvg/LightGlue's ``lightglue.LightGlue`` (reference
``lightglue/__init__.py:4``): same constructor, same ``forward({'image0','image1'})`` dict API, all
arithmetic in hand-written HIP kernels behind the C ABI of ``include/lightglue_amd.h``.
SURVEY.md §8 f3: the SuperPoint extractor (conv stack, keypoint extraction, descriptor head) runs on the same library
(``lightglue_amd.SuperPoint``), and so does ALIKED (``lightglue_amd.ALIKED``, aliked-n16 / n32).  The resize in front of them (the reference's ``ImagePreprocessor``) is ``lightglue_amd.ImagePreprocessor``, one HIP kernel.  SIFT feature stores (uint8 descriptors, RootSIFT, ``filter_dog_point``: ``lightglue_amd.sift``) are read as stored, and ``lightglue_amd.NearestNeighborMatcher`` matches any of these stores without weights (mutual nearest neighbour, ratio and distance tests); the SIFT detector itself, other extractors, image file I/O and visualisation are out of scope.
"""
from .lightglue import LightGlue  # noqa: F401
from .nn_matcher import NearestNeighborMatcher  # noqa: F401
from .twoview import TwoViewVerifier  # noqa: F401
from .relpose import RelativePoseEstimator  # noqa: F401
from .abspose import AbsolutePoseEstimator  # noqa: F401
from .triangulate import Triangulator  # noqa: F401
from .bundle import BundleAdjuster  # noqa: F401
from .posegraph import GlobalPoseEstimator  # noqa: F401
from .positioning import GlobalPositioner  # noqa: F401
from .superpoint import SuperPoint, plan_image_batches  # noqa: F401
from .aliked import ALIKED  # noqa: F401
from .preprocess import ImagePreprocessor, numpy_image_to_torch  # noqa: F401
from .parallel import PairShardedMatcher, shard_range  # noqa: F401
from .inflight import InflightMatcher  # noqa: F401
from .sift import filter_dog_point, sift_features, sift_to_rootsift  # noqa: F401
from .glue import batch_to_device, cm_prune, collate_features, extracted_to_image_frame, match_batch, match_pair, match_pairs, prefetch_to_device, rbd, verify_pairs, estimate_poses, estimate_absolute_poses, triangulate_tracks, bundle_adjust, estimate_global_poses, position_from_tracks  # noqa: F401

__all__ = ["LightGlue", "NearestNeighborMatcher", "TwoViewVerifier", "verify_pairs", "RelativePoseEstimator", "estimate_poses", "AbsolutePoseEstimator", "estimate_absolute_poses", "Triangulator", "triangulate_tracks", "BundleAdjuster", "bundle_adjust", "GlobalPoseEstimator", "estimate_global_poses", "GlobalPositioner", "position_from_tracks", "SuperPoint", "ALIKED", "ImagePreprocessor", "numpy_image_to_torch", "PairShardedMatcher", "InflightMatcher", "shard_range", "match_pair", "match_batch", "match_pairs", "collate_features", "extracted_to_image_frame", "rbd", "cm_prune",
           "batch_to_device", "prefetch_to_device", "plan_image_batches", "sift_to_rootsift", "filter_dog_point", "sift_features"]
__version__ = "0.2.0"
