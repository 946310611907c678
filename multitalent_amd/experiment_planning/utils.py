"""The first step of `nnUNet_plan_and_preprocess` (reference experiment_planning/utils.py:82-135): the file lists of a raw task
folder from its `dataset.json`, and `crop`, which runs the offline cropper of `preprocessing/device_cropping.py` on them."""
import json
import os
import shutil

from .. import paths
from ..preprocessing.device_cropping import ImageCropper


def create_lists_from_splitted_dataset(base_folder_splitted):
    """-> ([[modality files ..., label file], ...] in the order of dataset.json's training list, {modality index: name})."""
    with open(os.path.join(base_folder_splitted, "dataset.json")) as f:
        d = json.load(f)
    num_modalities = len(d['modality'].keys())
    lists = []
    for tr in d['training']:
        case = tr['image'].split("/")[-1][:-7]
        cur_pat = [os.path.join(base_folder_splitted, "imagesTr", case + "_%04.0d.nii.gz" % mod) for mod in range(num_modalities)]
        cur_pat.append(os.path.join(base_folder_splitted, "labelsTr", tr['label'].split("/")[-1]))
        lists.append(cur_pat)
    return lists, {int(i): d['modality'][str(i)] for i in d['modality'].keys()}


def crop(task_string, override=False, num_threads=paths.default_num_threads):
    """Crops every training case of the raw task to its non-zero region into nnUNet_cropped_data/<task>; a case whose files
    exist is skipped unless `override`, which first removes the whole folder."""
    raw = os.path.join(paths.require(paths.nnUNet_raw_data), task_string)
    cropped_out_dir = os.path.join(paths.require(paths.nnUNet_cropped_data), task_string)
    os.makedirs(cropped_out_dir, exist_ok=True)
    if override and os.path.isdir(cropped_out_dir):
        shutil.rmtree(cropped_out_dir)
        os.makedirs(cropped_out_dir, exist_ok=True)
    lists, _ = create_lists_from_splitted_dataset(raw)
    imgcrop = ImageCropper(num_threads, cropped_out_dir)
    imgcrop.run_cropping(lists, overwrite_existing=override)
    shutil.copy(os.path.join(raw, "dataset.json"), cropped_out_dir)
