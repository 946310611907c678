"""`Task100_MultiTalent_addregions` (reference nnunet/dataset_conversion/Task100_MultiTalent_addregions.py:7-36): after cropping
and preprocessing, every case `.pkl` of `nnUNet_cropped_data/<task>` and of every sub-folder of `nnUNet_preprocessed/<task>` gets
`valid_labels` and `valid_regions`, which `MultiTalent_trainer_ddp` reads from each case.  They come from the `_tr` dictionaries of
the `cases_have_regions_labels.pkl` that the conversion wrote into the raw task, under `<case>.nii.gz`.  Host only."""
import os
import pickle
import sys

from .. import paths

NOT_A_CASE = ('dataset_properties.pkl', 'intensityproperties.pkl')


def _case_pickles(folder):
    return sorted(f for f in os.listdir(folder) if f.endswith('.pkl') and f not in NOT_A_CASE and os.path.isfile(os.path.join(folder, f)))


def _add(folder, labels_tr, regions_tr):
    n = 0
    for p in _case_pickles(folder):
        key = p[:-4] + '.nii.gz'
        with open(os.path.join(folder, p), 'rb') as f:
            content = pickle.load(f)
        content['valid_labels'] = labels_tr[key]                 # KeyError: a case the conversion does not know
        content['valid_regions'] = regions_tr[key]
        with open(os.path.join(folder, p), 'wb') as f:
            pickle.dump(content, f)
        n += 1
    return n


def add_regions(task_name="Task100_MultiTalent"):
    """-> the number of case files written."""
    with open(os.path.join(paths.require(paths.nnUNet_raw_data), task_name, 'cases_have_regions_labels.pkl'), 'rb') as f:
        labels_tr, _, _, regions_tr, _, _ = pickle.load(f)
    n = _add(os.path.join(paths.require(paths.nnUNet_cropped_data), task_name), labels_tr, regions_tr)
    preprocessed = os.path.join(paths.require(paths.preprocessing_output_dir), task_name)
    for d in sorted(os.listdir(preprocessed)):
        if os.path.isdir(os.path.join(preprocessed, d)):
            n += _add(os.path.join(preprocessed, d), labels_tr, regions_tr)
    return n


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Add valid_labels / valid_regions to every cropped and preprocessed case of Task100.")
    ap.add_argument('--task_name', default="Task100_MultiTalent")
    a = ap.parse_args(argv)
    print("%s: %d case files updated" % (a.task_name, add_regions(a.task_name)))


if __name__ == '__main__':
    main(sys.argv[1:])
