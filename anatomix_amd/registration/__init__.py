from .sliding_window import sliding_window_inference, window_starts, importance_map  # noqa: F401
from .convex_adam_utils import (minmax, extract_features, load_model, MINDSSC, apply_avg_pool3d,  # noqa: F401
                                smooth_merged_features, correlate, stage1_inputs, coupled_convex,
                                coupled_convex_step, inverse_consistency, resize_trilinear, generate_grid,
                                JacobianDet, jacobian_determinant, jacobian_statistics, JACOBIAN_STATS)
from .instance_optimization import (merge_features, run_stage1_registration, create_warp, run_instance_opt,  # noqa: F401
                                    instance_opt_grad, instance_opt, instance_opt_smooth3, instance_opt_adam_step,
                                    warp_volume)
from .metrics import label_overlap, dice_score, dice_from_counts  # noqa: F401
from .run_convex_adam_with_network_feats import register_volumes, convex_adam, result_names, build_parser  # noqa: F401
