"""pixsfm-compatible Python surface of the accelerated KA/BA path (same class / method names as
pixsfm.keypoint_adjustment, pixsfm.bundle_adjustment, pixsfm._pixsfm._base/_features)."""
from . import base, extract, features, localization, reconstruction, triangulation, two_view  # noqa: F401
from . import homography  # noqa: F401,E402
from . import fundamental  # noqa: F401,E402
from .bundle_adjustment import (BundleAdjuster, BundleAdjustmentSetup, CostMapBundleAdjuster,  # noqa: F401
                                CostMapBundleOptimizer, CostMapExtractor, FeatureReferenceBundleAdjuster,
                                FeatureReferenceBundleOptimizer, FeatureView, GeometricBundleAdjuster,
                                GeometricBundleOptimizer, ReferenceExtractor, default_problem_setup)
from .keypoint_adjustment import (FeatureMetricKeypointAdjuster, FeatureMetricKeypointOptimizer,  # noqa: F401
                                  KeypointAdjuster, KeypointAdjustmentSetup,
                                  TopologicalReferenceKeypointAdjuster, TopologicalReferenceKeypointOptimizer,
                                  build_matching_graph, find_problem_labels)
from .localization import (QueryBundleAdjuster, QueryBundleOptimizer, QueryKeypointAdjuster,  # noqa: F401,E402
                           QueryKeypointOptimizer, QueryLocalizer, absolute_pose_estimation,  # noqa: F401,E402
                           absolute_pose_estimation_batch, compute_reprojection_errors, find_feature_inliers,  # noqa: F401,E402
                           find_nearest_references, find_unique_inliers, find_unique_min_by_group,  # noqa: F401,E402
                           find_unique_min_reproj_inliers)  # noqa: F401,E402
from .extract import (FeatureExtractor, extract_patchdata_from_graph, features_from_graph,  # noqa: F401,E402
                      features_from_image_list, features_from_reconstruction)
from .triangulation import TrackTriangulator  # noqa: F401,E402
from .matching import DescriptorMatcher, guided_model, guided_threshold, pairs_2d3d_from_matches  # noqa: F401,E402
from .two_view import TwoViewVerifier, essential_matrix_estimation  # noqa: F401,E402
from .homography import TwoViewClassifier, homography_matrix_estimation, two_view_config  # noqa: F401,E402
from .fundamental import fundamental_matrix_estimation, two_view_config_uncalibrated  # noqa: F401,E402
from . import mapping  # noqa: F401,E402
from .mapping import IncrementalMapper  # noqa: F401,E402
from . import global_mapping  # noqa: F401,E402
from .global_mapping import GlobalMapper, rotation_averaging  # noqa: F401,E402
from . import sift  # noqa: F401,E402
from .sift import SiftExtractor  # noqa: F401,E402
from . import retrieval  # noqa: F401,E402
from .retrieval import (GlobalDescriptorExtractor, pairs_from_exhaustive, pairs_from_retrieval,  # noqa: F401,E402
                        unique_pairs)
from . import map_localization  # noqa: F401,E402
from .map_localization import MapLocalizer, covisibility_clustering, pairs_from_covisibility  # noqa: F401,E402
from . import covariance  # noqa: F401,E402
from .covariance import BACovariance, estimate_ba_covariance  # noqa: F401,E402
from . import evaluation  # noqa: F401,E402
from .evaluation import (Sim3, align_reconstructions, compare_reconstructions, compute_auc, compute_pose_error,  # noqa: F401,E402
                         compute_recall, evaluate_point_cloud, export_PLY, read_ply_points)
