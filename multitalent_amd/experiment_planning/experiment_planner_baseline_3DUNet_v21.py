"""`ExperimentPlanner3D_v21` (reference experiment_planning/experiment_planner_baseline_3DUNet_v21.py): the planner behind
`nnUNetPlansv2.1`.  Against the base planner: 32 base features (with the budget scaled by 32 / 30, so the patch is planned as for
30), pooling that follows the spacing, and a target spacing that does not take the median along a strongly anisotropic axis."""
import os

import numpy as np

from ..network_architecture.generic_UNet import Generic_UNet
from .common_utils import get_pool_and_conv_props
from .experiment_planner_baseline_3DUNet import ExperimentPlanner


class ExperimentPlanner3D_v21(ExperimentPlanner):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner3D_v21, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "nnUNetData_plans_v2.1"
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "nnUNetPlansv2.1_plans_3D.pkl")
        self.unet_base_num_features = 32

    def get_target_spacing(self):
        """The median spacing; but where the coarsest axis is more than 3 times coarser than the others AND has less than a third
        of their voxels (cine MRI: (10, 1.5, 1.5)), that axis takes the 10th percentile of its spacings, so that the cases with
        the fewest slices are not resampled far; it never becomes finer than the other axes."""
        spacings = self.dataset_properties['all_spacings']
        sizes = self.dataset_properties['all_sizes']
        target = np.percentile(np.vstack(spacings), self.target_spacing_percentile, 0)
        target_size = np.percentile(np.vstack(sizes), self.target_spacing_percentile, 0)
        worst_spacing_axis = np.argmax(target)
        other_axes = [i for i in range(len(target)) if i != worst_spacing_axis]
        other_spacings = [target[i] for i in other_axes]
        other_sizes = [target_size[i] for i in other_axes]
        has_aniso_spacing = target[worst_spacing_axis] > (self.anisotropy_threshold * max(other_spacings))
        has_aniso_voxels = target_size[worst_spacing_axis] * self.anisotropy_threshold < min(other_sizes)
        if has_aniso_spacing and has_aniso_voxels:
            spacings_of_that_axis = np.vstack(spacings)[:, worst_spacing_axis]
            target_spacing_of_that_axis = np.percentile(spacings_of_that_axis, 10)
            if target_spacing_of_that_axis < max(other_spacings):
                target_spacing_of_that_axis = max(max(other_spacings), target_spacing_of_that_axis) + 1e-5
            target[worst_spacing_axis] = target_spacing_of_that_axis
        return target

    def topology(self, spacing, patch_size):
        return get_pool_and_conv_props(spacing, patch_size, self.unet_featuremap_min_edge_length, self.unet_max_numpool)

    def vram_budget(self):
        return Generic_UNet.use_this_for_batch_size_computation_3D * self.unet_base_num_features / \
               Generic_UNet.BASE_NUM_FEATURES_3D
