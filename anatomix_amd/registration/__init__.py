from .sliding_window import sliding_window_inference, window_starts, importance_map  # noqa: F401
from .convex_adam_utils import (minmax, extract_features, load_model, MINDSSC, apply_avg_pool3d,  # noqa: F401
                                smooth_merged_features, correlate, stage1_inputs, coupled_convex,
                                coupled_convex_step, inverse_consistency, resize_trilinear)
from .instance_optimization import (merge_features, run_stage1_registration, create_warp, run_instance_opt,  # noqa: F401
                                    instance_opt_grad, instance_opt, instance_opt_smooth3, instance_opt_adam_step,
                                    warp_volume)
