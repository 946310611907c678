"""Ensembling of two trained configurations on their cross-validation outputs (reference
nnunet/evaluation/model_selection/ensemble.py:26-123): the validation probabilities (`--npz`) of both models are averaged case by
case, the merged masks are scored against the ground truth and a postprocessing is determined for the ensemble.  The average and
the label decision are `mt_ensemble_classify` (through `inference.ensemble_predictions`), scoring and the connected-component
search are the device paths of `aggregate_scores` and `determine_postprocessing`."""
import json
import os
import pickle
import shutil


from ...inference.ensemble_predictions import _load_case, merge_on_device
from ...postprocessing.connected_components import default_num_threads, determine_postprocessing
from ...run.default_configuration import network_training_output_dir, preprocessing_output_dir
from ..evaluator import aggregate_scores


def merge(args):
    """reference :26-36: (file1, file2, properties_file, out_file); the mean of the two members, argmax, the geometry of the
    properties file.  An existing out_file is kept."""
    from ...utilities.nifti_io import write_image
    file1, file2, properties_file, out_file = args
    if not os.path.isfile(out_file):
        arrays, props, _ = _load_case([file1, file2], [properties_file])
        seg, _ = merge_on_device(arrays, props[0], None, keep_on_device=out_file.endswith('.nii.gz'))
        write_image(seg, out_file, props[0]['itk_spacing'], props[0]['itk_origin'], props[0]['itk_direction'])


def _subfiles(folder, suffix):
    return sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(suffix))


def ensemble(training_output_folder1, training_output_folder2, output_folder, task, validation_folder, folds, allow_ensembling=True):
    """reference :39-123."""
    print("\nEnsembling folders\n", training_output_folder1, "\n", training_output_folder2)
    output_folder_base = output_folder
    output_folder = os.path.join(output_folder_base, "ensembled_raw")
    dataset_directory = os.path.join(preprocessing_output_dir(), task)
    with open(os.path.join(training_output_folder1, "plans.pkl"), 'rb') as f:
        plans = pickle.load(f)                                        # only for the labels
    folder_with_gt_segs = os.path.join(dataset_directory, "gt_segmentations")
    jobs, out_files, gt_segmentations = [], [], []
    rerun = "Please rerun validation with `nnUNet_train CONFIG TRAINER TASK FOLD -val --npz`"
    for f in folds:
        nets = [os.path.join(t, "fold_%d" % f, validation_folder) for t in (training_output_folder1, training_output_folder2)]
        for v in nets:
            if not os.path.isdir(v):
                raise AssertionError("Validation directory missing: %s. %s" % (v, rerun))
        # a finished validation has left its summary.json
        if not os.path.isfile(os.path.join(nets[0], 'summary.json')):
            raise AssertionError("Validation directory incomplete: %s. %s" % (nets[0], rerun))
        if not os.path.isfile(os.path.join(nets[1], 'summary.json')):
            raise AssertionError("Validation directory missing: %s. %s" % (nets[1], rerun))
        ids_npz = [sorted(i[:-4] for i in _subfiles(v, 'npz')) for v in nets]
        for v, npz in zip(nets, ids_npz):
            ids_nii = [i[:-7] for i in _subfiles(v, 'nii.gz')
                       if not i.endswith("noPostProcess.nii.gz") and not i.endswith('_postprocessed.nii.gz')]
            if not all([i in npz for i in ids_nii]):
                raise AssertionError("Missing npz files in folder %s. Please run the validation for all models and folds with the "
                                     "'--npz' flag." % v)
        assert all([i == j for i, j in zip(*ids_npz)]), "npz filenames do not match. This should not happen."
        os.makedirs(output_folder, exist_ok=True)
        for p in ids_npz[0]:
            jobs.append((os.path.join(nets[0], p + '.npz'), os.path.join(nets[1], p + '.npz'), os.path.join(nets[0], p) + ".pkl",
                         os.path.join(output_folder, p + ".nii.gz")))
            out_files.append(jobs[-1][3])
            gt_segmentations.append(os.path.join(folder_with_gt_segs, p + ".nii.gz"))
    for j in jobs:
        merge(j)

    if not os.path.isfile(os.path.join(output_folder, "summary.json")) and len(out_files) > 0:
        aggregate_scores(tuple(zip(out_files, gt_segmentations)), labels=plans['all_classes'],
                         json_output_file=os.path.join(output_folder, "summary.json"), json_task=task,
                         json_name=task + "__" + output_folder_base.split("/")[-1], num_threads=default_num_threads)

    if allow_ensembling and not os.path.isfile(os.path.join(output_folder_base, "postprocessing.json")):
        # the postprocessing of the cross-validations does not carry over to the ensemble: it is determined again
        determine_postprocessing(output_folder_base, folder_with_gt_segs, "ensembled_raw", "temp", "ensembled_postprocessed",
                                 default_num_threads, dice_threshold=0)
        out_dir_all_json = os.path.join(network_training_output_dir(), "summary_jsons")
        summary = os.path.join(output_folder_base, "ensembled_postprocessed", "summary.json")
        with open(summary) as f:
            json_out = json.load(f)
        json_out["experiment_name"] = output_folder_base.split("/")[-1]
        with open(summary, 'w') as f:
            json.dump(json_out, f, sort_keys=True, indent=4)
        os.makedirs(out_dir_all_json, exist_ok=True)
        shutil.copy(summary, os.path.join(out_dir_all_json, "%s__%s.json" % (task, output_folder_base.split("/")[-1])))
