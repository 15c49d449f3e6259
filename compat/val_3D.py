"""`from val_3D import test_all_case_base` / `test_all_case_amos` (train_inherent_consistent_*_3D_*.py) -> icl_amd.val_3D."""
from icl_amd.val_3D import *  # noqa: F401,F403
from icl_amd.val_3D import (binary_asd, binary_assd, binary_hd, binary_hd95, binary_nsd, cal_metric,  # noqa: F401
                            cal_metric_multiclass, components_mode, keep_components, sliding_window_inference,
                            surface_metrics_multiclass, test_all_case_amos, test_all_case_base, test_single_case_base)
