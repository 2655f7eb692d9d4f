"""viorb_amd — MI355X-native per-frame front-end for VIORB (ORB extract / match / IMU / pose solve).

The product is libviorb_hip.so (HIP kernels behind the C ABI of include/viorb.h). This package is the
thin Python mirror of the reference's C++ interface used by tests and bench.py; it has no CPU
fallback: if the library is missing, `viorb_amd.lib()` raises.
"""
from .capi import lib, ViorbError, KP_DTYPE  # noqa: F401
from .extractor import ORBextractor  # noqa: F401
from .frontend import Frontend, ORBmatcher, PoseOptimization, PoseOptimizationSE3, LocalBundleAdjustmentNavState, LocalBundleAdjustmentNavStateBatch, LocalBundleAdjustment, LocalBundleAdjustmentBatch, ORBVocabulary, SearchByBoW, SearchForTriangulation, Fuse, preintegrate, descriptor_distance, match_bruteforce, SearchLocalPoints, UndistortKeyPoints, ComputeImageBounds  # noqa: F401
from .mapping import TriangulatePairs, TriangulatePairsBatch, MapPointUpdate, CreateNewMapPoints, CreateNewMapPointsHost, mapping_camera  # noqa: F401
from .vi_init import PreintegrateIntervals, PreintegrateIntervalsBatch, OptimizeInitialGyroBias, ViInit, ViInitHost, ViInitApplyHost, vi_config, unpack_est  # noqa: F401
from .global_ba import GlobalBundleAdjustmentNavState, GlobalBundleAdjustmentNavStateDevice, gba_workspace_bytes, GlobalBundleAdjustmentSE3, GlobalBundleAdjustmentSE3Device, gba_se3_workspace_bytes  # noqa: F401
from .place import BowVector, BowVector_device, BowScore, BowScorePairs, KeyFrameDatabase, pack_bows  # noqa: F401
from .two_view import TwoViewInit, TwoViewBatch, draw_sets, two_view_config  # noqa: F401
from .sim3 import Sim3Batch, sim3_ransac, sim3_config, optimize_sim3, optimize_sim3_batch, ransac_iterations  # noqa: F401
from .sim3_match import Sim3MatchBatch, search_by_sim3, search_by_projection_sim3, fuse_sim3, keyframe_grid  # noqa: F401
from .relocalization import RelocBatch, search_by_projection_reloc  # noqa: F401
from .search_init import SearchInitBatch, search_for_initialization, scene_median_depth, scene_median_depth_batch  # noqa: F401
from .culling import CullBatch, key_frame_culling, map_point_culling, map_point_culling_batch  # noqa: F401
from .local_map import LocalMapBatch, update_local_map  # noqa: F401
from .covisibility import CovisBatch, update_connections  # noqa: F401
from .kf_removal import KfRemovalBatch, remove_key_frames  # noqa: F401
from .map_fusion import FuseBatch, apply_fuse  # noqa: F401
from .map_correction import CorrectLoopBatch, correct_loop, ApplyGbaBatch, apply_global_ba  # noqa: F401
from .essential_graph import OptimizeEssentialGraph, OptimizeEssentialGraphDevice, essential_graph_workspace_bytes  # noqa: F401
from .sim3 import draw_sets as sim3_draw_sets  # noqa: F401  (draw_sets is the two-view initialiser's)
