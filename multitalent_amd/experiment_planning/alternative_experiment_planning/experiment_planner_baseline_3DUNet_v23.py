"""`ExperimentPlanner3D_v23` (reference experiment_planning/alternative_experiment_planning/experiment_planner_baseline_3DUNet_v23.py):
the v2.1 plans with `Preprocessor3DDifferentResampling` — order 3 along the anisotropic axis for the data and order 1 for the
labels, where the default preprocessor takes order 0 there.

    python -m multitalent_amd.experiment_planning.nnUNet_plan_and_preprocess -t 9 -pl3d ExperimentPlanner3D_v23 -pl2d None"""
import os

from ..experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21


class ExperimentPlanner3D_v23(ExperimentPlanner3D_v21):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        super(ExperimentPlanner3D_v23, self).__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.data_identifier = "nnUNetData_plans_v2.3"
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "nnUNetPlansv2.3_plans_3D.pkl")
        self.preprocessor_name = "Preprocessor3DDifferentResampling"
