from .matrices import AVAILABLE_ROTATIONS, AVAILABLE_UNITS, translation_matrix, rotation_matrix, shear_matrix, \
    scale_matrix, transform_matrix, box_matrices, place_matrices, tilt_matrices, backproject_matrices, \
    backproject_box_matrices, grid_nodes, stack_matrices, stack_grid_nodes
from .filters import AVAILABLE_WINDOWS, ramp_taps
from .correlation import patch_bounds, peak_shifts, patch_moments, normalized_scores
from .general import compute_prefilter_workgroup_dims, compute_elementwise_launch_dims, get_available_devices, \
    switch_to_device, parse_device, compute_post_transform_dimensions
