"""`ExperimentPlanner3D_v21_MultiTalent` (reference task_specific_planner/MultiTalent/MultiTalent_planner.py:33-131): the plan of
the MultiTalent collection, Task100.  v2.1's pooling and anisotropy-free fixed spacing (1.5, 1, 1), a budget of 15/8 of the
standard one for larger patches, and batch size 4 whatever the budget leaves.  Its constructor runs the BASE planner's, not
v2.1's, so the network has 30 base features, and the budget is not scaled by 32 / 30."""
import os

import numpy as np

from ....network_architecture.generic_UNet import Generic_UNet
from ...experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21


class ExperimentPlanner3D_v21_MultiTalent(ExperimentPlanner3D_v21):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner3D_v21, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "MultiTalent_data"
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "MultiTalent_bs4_plans_3D.pkl")

    def get_target_spacing(self):
        return np.array([1.5, 1, 1])

    def vram_budget(self):
        return Generic_UNet.use_this_for_batch_size_computation_3D * 15 / 8

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        plan = super().get_properties_for_stage(current_spacing, original_spacing, original_shape, num_cases, num_modalities,
                                                num_classes)
        plan['batch_size'] = 4
        return plan
