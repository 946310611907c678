"""`nnUNet_plan_and_preprocess` (reference experiment_planning/nnUNet_plan_and_preprocess.py:27-166): from a raw task folder to
plans and preprocessed training cases.  Per task: verify (optional), crop, fingerprint, copy `dataset_properties.pkl` and
`dataset.json`, plan, preprocess (unless `-no_pp`).  Every stage that touches voxels runs on the device (`sanity_checks`,
`device_cropping.ImageCropper`, `DatasetAnalyzer`, `GenericPreprocessor.run`); planning is host arithmetic.

The 2D planners are not part of this package: pass `-pl2d None`.

    python -m multitalent_amd.experiment_planning.nnUNet_plan_and_preprocess -t 100 \\
        -pl3d ExperimentPlanner3D_v21_MultiTalent -pl2d None -tf 16 --verify_dataset_integrity"""
import argparse
import json
import os
import shutil

import multitalent_amd
from .. import paths
from ..preprocessing.sanity_checks import verify_dataset_integrity
from ..training.model_restore import recursive_find_python_class
from ..utilities.task_name_id_conversion import convert_id_to_task_name
from .DatasetAnalyzer import DatasetAnalyzer
from .utils import crop


def _parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("-t", "--task_ids", nargs="+", help="task ids; each needs a folder 'TaskXXX_...' in the raw data folder")
    parser.add_argument("-pl3d", "--planner3d", type=str, default="ExperimentPlanner3D_v21",
                        help="class name of the 3D planner, or 'None'")
    parser.add_argument("-pl2d", "--planner2d", type=str, default="ExperimentPlanner2D_v21",
                        help="the 2D planners are not part of this package: pass '-pl2d None'")
    parser.add_argument("-no_pp", action="store_true", help="plan only, do not preprocess")
    parser.add_argument("-tl", type=int, required=False, default=8, help="host threads writing the low resolution stage")
    parser.add_argument("-tf", type=int, required=False, default=8,
                        help="host threads reading ahead of and writing behind the device (cropping, full resolution stage)")
    parser.add_argument("--verify_dataset_integrity", required=False, default=False, action="store_true",
                        help="check the dataset first; do this once for each dataset")
    parser.add_argument("-overwrite_plans", type=str, default=None, required=False,
                        help="a plans file (same number of modalities) to use instead of this dataset's own plan, for fine-tuning "
                             "pretrained weights; requires -pl3d ExperimentPlanner3D_v21_Pretrained")
    parser.add_argument("-overwrite_plans_identifier", type=str, default=None, required=False,
                        help="with -overwrite_plans: IDENTIFIER of plans and data; train with -p nnUNetPlans_pretrained_IDENTIFIER")
    return parser


def _find_planner(name):
    search_in = os.path.join(multitalent_amd.__path__[0], "experiment_planning")
    planner = recursive_find_python_class([search_in], name, current_module="multitalent_amd.experiment_planning")
    if planner is None:
        raise RuntimeError("Could not find the Planner class %s. Make sure it is located somewhere in "
                           "multitalent_amd.experiment_planning" % name)
    return planner


def main(argv=None):
    args = _parser().parse_args(argv)
    planner_name3d = None if args.planner3d == "None" else args.planner3d
    planner_name2d = None if args.planner2d == "None" else args.planner2d

    # refusals come before any file is touched
    if args.overwrite_plans is not None:
        assert planner_name3d == 'ExperimentPlanner3D_v21_Pretrained', "When using --overwrite_plans you need to use " \
                                                                       "'-pl3d ExperimentPlanner3D_v21_Pretrained'"
        assert args.overwrite_plans_identifier is not None, "You need to specify -overwrite_plans_identifier"
    if planner_name2d is not None:
        raise NotImplementedError("the 2D planners (-pl2d %s) are not part of multitalent_amd, which is 3D only: pass '-pl2d None'"
                                  % planner_name2d)
    planner_3d = _find_planner(planner_name3d) if planner_name3d is not None else None

    raw = paths.require(paths.nnUNet_raw_data)
    tasks = []
    for i in args.task_ids:
        task_name = convert_id_to_task_name(int(i))
        if args.verify_dataset_integrity:
            verify_dataset_integrity(os.path.join(raw, task_name))
        crop(task_name, False, args.tf)
        tasks.append(task_name)

    for t in tasks:
        print("\n\n\n", t)
        cropped_out_dir = os.path.join(paths.require(paths.nnUNet_cropped_data), t)
        preprocessing_output_dir_this_task = os.path.join(paths.require(paths.preprocessing_output_dir), t)

        # the intensity properties are collected only where a modality is CT
        with open(os.path.join(cropped_out_dir, 'dataset.json')) as f:
            modalities = list(json.load(f)["modality"].values())
        collect_intensityproperties = ("CT" in modalities) or ("ct" in modalities)
        dataset_analyzer = DatasetAnalyzer(cropped_out_dir, overwrite=False, num_processes=args.tf)
        dataset_analyzer.analyze_dataset(collect_intensityproperties)

        os.makedirs(preprocessing_output_dir_this_task, exist_ok=True)
        shutil.copy(os.path.join(cropped_out_dir, "dataset_properties.pkl"), preprocessing_output_dir_this_task)
        shutil.copy(os.path.join(raw, t, "dataset.json"), preprocessing_output_dir_this_task)

        threads = (args.tl, args.tf)
        print("number of threads: ", threads, "\n")
        if planner_3d is not None:
            if args.overwrite_plans is not None:
                exp_planner = planner_3d(cropped_out_dir, preprocessing_output_dir_this_task, args.overwrite_plans,
                                         args.overwrite_plans_identifier)
            else:
                exp_planner = planner_3d(cropped_out_dir, preprocessing_output_dir_this_task)
            exp_planner.plan_experiment()
            if not args.no_pp:
                exp_planner.run_preprocessing(threads)


if __name__ == "__main__":
    main()
