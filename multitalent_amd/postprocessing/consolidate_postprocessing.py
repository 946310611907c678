"""`consolidate_folds` (reference nnunet/postprocessing/consolidate_postprocessing.py:25-97): after the cross-validation, the
validation masks of all folds are collected in `<model>/cv_niftis_raw`, scored against `<model>/gt_niftis`, and ONE
postprocessing is determined for the experiment: the `<model>/postprocessing.json` that `predict_cases` applies.  Scoring
(`aggregate_scores`) and the connected-component search (`determine_postprocessing`) run on the device."""
import argparse
import json
import os
import shutil

from ..evaluation.evaluator import aggregate_scores
from .connected_components import default_num_threads, determine_postprocessing


def _niftis(folder):
    return sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(".nii.gz"))


def collect_cv_niftis(cv_folder, output_folder, validation_folder_name='validation_raw', folds=(0, 1, 2, 3, 4)):
    """reference :25-40: copy every fold's validation masks into `output_folder`."""
    validation_raw_folders = [os.path.join(cv_folder, "fold_%d" % i, validation_folder_name) for i in folds]
    exist = [os.path.isdir(i) for i in validation_raw_folders]
    if not all(exist):
        raise RuntimeError("some folds are missing. Please run the full 5-fold cross-validation. "
                           "The following folds seem to be missing: %s" % [i for j, i in enumerate(folds) if not exist[j]])
    os.makedirs(output_folder, exist_ok=True)
    # (the reference indexes the folder list with the fold NUMBER, :38, which only works for folds 0..n-1 in order)
    for folder in validation_raw_folders:
        for n in _niftis(folder):
            shutil.copy(os.path.join(folder, n), output_folder)


def consolidate_folds(output_folder_base, validation_folder_name='validation_raw', advanced_postprocessing=False,
                      folds=(0, 1, 2, 3, 4)):
    """reference :43-85.  output_folder_base: the experiment's output folder (fold_0, fold_1, ... and gt_niftis inside)."""
    output_folder_raw = os.path.join(output_folder_base, "cv_niftis_raw")
    if os.path.isdir(output_folder_raw):
        shutil.rmtree(output_folder_raw)
    output_folder_gt = os.path.join(output_folder_base, "gt_niftis")
    collect_cv_niftis(output_folder_base, output_folder_raw, validation_folder_name, folds)
    niftis = _niftis(output_folder_raw)
    if len(niftis) != len(_niftis(output_folder_gt)):
        raise AssertionError("If does not seem like you trained all the folds! Train all folds first!")
    # the class labels to expect come from a fold's summary
    with open(os.path.join(output_folder_base, "fold_0", validation_folder_name, "summary.json")) as f:
        classes = [int(i) for i in json.load(f)['results']['mean'].keys()]
    test_pred_pairs = [(os.path.join(output_folder_raw, i), os.path.join(output_folder_gt, i)) for i in niftis]
    # determine_postprocessing wants a summary.json next to the raw predictions
    aggregate_scores(test_pred_pairs, labels=classes, json_output_file=os.path.join(output_folder_raw, "summary.json"),
                     num_threads=default_num_threads)
    determine_postprocessing(output_folder_base, output_folder_gt, 'cv_niftis_raw', final_subf_name="cv_niftis_postprocessed",
                             processes=default_num_threads, advanced_postprocessing=advanced_postprocessing)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-f", type=str, required=True, help="the experiment's output folder (fold_0, fold_1, ... are its subfolders)")
    consolidate_folds(ap.parse_args(argv).f)


if __name__ == "__main__":
    main()
