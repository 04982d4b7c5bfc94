"""dkg_amd — MI355X-native Discrete Knowledge Gradient (quasirandom/decoupled-kg hot path).

Drop-in for ``decoupledbo.modules.acquisition.discretekg``; the arithmetic runs
in hand-written HIP kernels for gfx950 behind the C ABI of ``include/dkg.h``.
"""

from .boxes import dominated_boxes, hypervolume_front
from .discretekg import (
    DiscreteKnowledgeGradient,
    calculate_discrete_kg,
    calculate_epigraph_indices,
    calculate_epigraph_indices_batched,
    calculate_expected_value_of_piecewise_linear_function,
    calculate_discrete_kg_conditioning_on_single_output,
    clear_state_cache,
    kg_from_lines,
    normalise_targets,
    t_batch_mode_transform,
)
from .errors import BotorchTensorDimensionError, DkgNativeError, UnsupportedError
from .gp_state import (
    DeviceGPState,
    gradient_rows,
    reset_state_stats,
    set_gradient_rows,
    set_incremental_state,
    state_stats,
)
from .hvkg import PosteriorMeanHypervolume, qHypervolumeKnowledgeGradient
from .jes import compute_sample_box_decomposition, qLowerBoundMultiObjectiveJointEntropySearch
from .jes_pareto import sample_discrete_pareto_optimal_points, sample_rff_paths
from .metrics import (
    calculate_reference_point,
    estimate_best_possible_expected_performance_after_scalarisation,
    estimate_expected_performance_after_scalarisation,
    estimate_hypervolume,
    estimate_hypervolume_from_posterior_mean,
)
from .model import ModelListGPState, SingleTaskGPState, from_botorch, from_state_dict
from .pareto import nondominated_rank, posterior_front_on_points, posterior_mean, sample_points_on_pareto_front
from .utils import is_power_of_2, make_torch_std_grid, sample_simplex

__all__ = [
    "DiscreteKnowledgeGradient",
    "calculate_discrete_kg",
    "calculate_epigraph_indices",
    "calculate_epigraph_indices_batched",
    "calculate_expected_value_of_piecewise_linear_function",
    "calculate_discrete_kg_conditioning_on_single_output",
    "clear_state_cache",
    "kg_from_lines",
    "qLowerBoundMultiObjectiveJointEntropySearch",
    "compute_sample_box_decomposition",
    "dominated_boxes",
    "hypervolume_front",
    "qHypervolumeKnowledgeGradient",
    "PosteriorMeanHypervolume",
    "normalise_targets",
    "t_batch_mode_transform",
    "BotorchTensorDimensionError",
    "DkgNativeError",
    "UnsupportedError",
    "DeviceGPState",
    "set_incremental_state",
    "set_gradient_rows",
    "gradient_rows",
    "state_stats",
    "reset_state_stats",
    "ModelListGPState",
    "SingleTaskGPState",
    "from_botorch",
    "from_state_dict",
    "posterior_mean",
    "nondominated_rank",
    "posterior_front_on_points",
    "sample_points_on_pareto_front",
    "sample_discrete_pareto_optimal_points",
    "sample_rff_paths",
    "calculate_reference_point",
    "estimate_best_possible_expected_performance_after_scalarisation",
    "estimate_expected_performance_after_scalarisation",
    "estimate_hypervolume",
    "estimate_hypervolume_from_posterior_mean",
    "is_power_of_2",
    "make_torch_std_grid",
    "sample_simplex",
]
