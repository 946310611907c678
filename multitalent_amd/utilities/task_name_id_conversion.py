"""`convert_id_to_task_name` / `convert_task_name_to_id` (reference utilities/task_name_id_conversion.py:21-68): the task folder
whose name starts with `Task<id>` among the raw, cropped, preprocessed and results roots; exactly one name must be found.  The
narrower lookup of `run/default_configuration.py` (preprocessed root only) stays what the training driver uses."""
import os

import numpy as np

from .. import paths


def _subdirs(folder, prefix):
    if not os.path.isdir(folder):            # the reference creates its roots when it is imported; here a missing root holds no task
        return []
    return sorted(d for d in os.listdir(folder) if d.startswith(prefix) and os.path.isdir(os.path.join(folder, d)))


def convert_id_to_task_name(task_id: int):
    startswith = "Task%03.0d" % task_id
    raw, cropped, preprocessed = paths.nnUNet_raw_data(), paths.nnUNet_cropped_data(), paths.preprocessing_output_dir()
    candidates = []
    for root in (cropped, preprocessed, raw):
        if root is not None:
            candidates += _subdirs(root, startswith)
    results = paths.network_training_output_dir()
    if results is not None:
        for m in ['2d', '3d_lowres', '3d_fullres', '3d_cascade_fullres']:
            if os.path.isdir(os.path.join(results, m)):
                candidates += _subdirs(os.path.join(results, m), startswith)
    unique_candidates = np.unique(candidates)
    if len(unique_candidates) > 1:
        raise RuntimeError("More than one task name found for task id %d. Please correct that. (I looked in the "
                           "following folders:\n%s\n%s\n%s" % (task_id, raw, preprocessed, cropped))
    if len(unique_candidates) == 0:
        env = [os.environ.get(k) if os.environ.get(k) is not None else 'None'
               for k in ('nnUNet_preprocessed', 'RESULTS_FOLDER', 'nnUNet_raw_data_base')]
        raise RuntimeError("Could not find a task with the ID %d. Make sure the requested task ID exists and that "
                           "nnU-Net knows where raw and preprocessed data are located (see Documentation - "
                           "Installation). Here are your currently defined folders:\nnnUNet_preprocessed=%s\nRESULTS_"
                           "FOLDER=%s\nnnUNet_raw_data_base=%s\nIf something is not right, adapt your environemnt "
                           "variables." % (task_id, *env))
    return str(unique_candidates[0])


def convert_task_name_to_id(task_name: str):
    assert task_name.startswith("Task")
    return int(task_name[4:7])
