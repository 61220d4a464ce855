from .clip_pseudolabels import compute_pseudo_labels, pseudolabel_top_k  # noqa: F401
from .compute_metrics import (adapter_path, evaluate_predictions, gda_head_path, linear_probe_path, load_parameters, save_parameters, save_predictions, save_pseudo_labels,  # noqa: F401
                              store_results, tip_cache_path)
