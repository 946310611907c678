"""`ExperimentPlanner3DFabiansResUNet_v21` (reference alternative_experiment_planning/experiment_planner_residual_3DUNet_v21.py):
v2.1's plan for the residual-encoder network `FabiansUNet` (`MultiTalent_meets_resenc`).  The pooling list gains a leading
[1, 1, 1] (the first encoder stage does not pool), each stage carries its number of residual blocks, and the budget and the
estimate are that network's.  Two things are the reference's and kept: the FIRST estimate is taken on the clipped start patch
before it is padded, and `run_preprocessing` does nothing, because the data is v2.1's (`nnUNetData_plans_v2.1`)."""
import os

from ...network_architecture.generic_modular_residual_UNet import FabiansUNet
from ..experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21


class ExperimentPlanner3DFabiansResUNet_v21(ExperimentPlanner3D_v21):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner3DFabiansResUNet_v21, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "nnUNetData_plans_v2.1"
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "nnUNetPlans_FabiansResUNet_v2.1_plans_3D.pkl")

    def vram_budget(self):
        return FabiansUNet.use_this_for_3D_configuration

    def default_batch_size(self):
        return FabiansUNet.default_min_batch_size

    @staticmethod
    def _blocks(pool_op_kernel_sizes):
        return (FabiansUNet.default_blocks_per_stage_encoder[:len(pool_op_kernel_sizes)],
                FabiansUNet.default_blocks_per_stage_decoder[:len(pool_op_kernel_sizes) - 1])

    def vram_estimate(self, patch_size, num_pool_per_axis, pool_op_kernel_sizes, num_modalities, num_classes):
        """pool_op_kernel_sizes: with the leading [1, 1, 1]."""
        encoder, decoder = self._blocks(pool_op_kernel_sizes)
        return FabiansUNet.compute_approx_vram_consumption(patch_size, self.unet_base_num_features, self.unet_max_num_filters,
                                                           num_modalities, num_classes, pool_op_kernel_sizes, encoder, decoder,
                                                           2, self.unet_min_batch_size)

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        new_median_shape, input_patch_size = self._median_shape_and_first_patch(current_spacing, original_spacing, original_shape)
        num_pool_per_axis, pool_kernels, conv_kernels, new_shp, divisible_by = self.topology(current_spacing, input_patch_size)
        pool_kernels = [[1, 1, 1]] + pool_kernels
        ref = self.vram_budget()
        here = self.vram_estimate(input_patch_size, num_pool_per_axis, pool_kernels, num_modalities, num_classes)
        while here > ref:
            num_pool_per_axis, pool_kernels, conv_kernels, new_shp, divisible_by = \
                self._shrink(current_spacing, new_shp, new_median_shape, divisible_by)
            pool_kernels = [[1, 1, 1]] + pool_kernels
            here = self.vram_estimate(new_shp, num_pool_per_axis, pool_kernels, num_modalities, num_classes)
        batch_size = self._batch_size(ref, here, self.default_batch_size(), new_median_shape, num_cases, new_shp)
        plan = self._stage_plan(batch_size, num_pool_per_axis, new_shp, new_median_shape, current_spacing, original_spacing,
                                pool_kernels, conv_kernels)
        plan['num_blocks_encoder'], plan['num_blocks_decoder'] = self._blocks(pool_kernels)
        return plan

    def run_preprocessing(self, num_threads):
        """Nothing to do: the preprocessed data is `ExperimentPlanner3D_v21`'s, under the same data identifier."""
        print("ExperimentPlanner3DFabiansResUNet_v21 reuses the data of ExperimentPlanner3D_v21 (%s); run that planner to "
              "preprocess" % self.data_identifier)
