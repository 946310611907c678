"""`ExperimentPlanner3D_v21_Pretrained` (reference alternative_experiment_planning/experiment_planner_pretrained.py): preprocess
a dataset with the plans of ANOTHER dataset, so that a network pretrained there fits (`-overwrite_plans`, fine-tuning with
`nnUNetTrainerV2_warmupsegheads`).  `plan_experiment` plans this dataset as v2.1 does and writes that; `run_preprocessing` first
replaces the plans by the given file, keeping this dataset's `num_classes`, and saves again under the same name.  Without the
preprocessing (`-no_pp`) the file on disk therefore holds this dataset's own plan, as in the reference."""
import os
import pickle

from ..experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21


class ExperimentPlanner3D_v21_Pretrained(ExperimentPlanner3D_v21):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder, pretrained_model_plans_file: str,
                 pretrained_name: str):
        super().__init__(folder_with_cropped_data, preprocessed_output_folder)
        self.pretrained_model_plans_file = pretrained_model_plans_file
        self.pretrained_name = pretrained_name
        self.data_identifier = "nnUNetData_pretrained_" + pretrained_name
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "nnUNetPlans_pretrained_%s_plans_3D.pkl" % pretrained_name)

    def load_pretrained_plans(self):
        classes = self.plans['num_classes']
        with open(self.pretrained_model_plans_file, 'rb') as f:
            self.plans = pickle.load(f)
        self.plans['num_classes'] = classes
        self.transpose_forward = self.plans['transpose_forward']
        self.preprocessor_name = self.plans['preprocessor_name']
        self.plans_per_stage = self.plans['plans_per_stage']
        self.plans['data_identifier'] = self.data_identifier
        self.save_my_plans()
        print(self.plans['plans_per_stage'])

    def run_preprocessing(self, num_threads):
        self.load_pretrained_plans()
        super().run_preprocessing(num_threads)
