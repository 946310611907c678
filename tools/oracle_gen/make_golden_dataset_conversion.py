"""Golden data of the dataset conversion from the REAL reference functions (runs only in the build container): the pure-numpy
`copy_and_convert_segmentation` (dataset_conversion/Task100_MultiTalent.py:229-275) and `generate_dataset_json`
(dataset_conversion/utils.py:27-76), imported through ref_import.  Writes tests/golden/dataset_conversion.npz (volumes as float64,
the array `get_fdata` hands the reference, and its uint8 results) and tests/golden/dataset_conversion.json (the cases, the value
the reference raises on, and the dataset.json of a fabricated folder)."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install()
import batchgenerators.utilities.file_and_folder_operations as ffo  # noqa: E402


def subfiles(folder, join=True, prefix=None, suffix=None, sort=True):
    """batchgenerators.utilities.file_and_folder_operations.subfiles (third party, restated)."""
    res = [os.path.join(folder, i) if join else i for i in os.listdir(folder)
           if os.path.isfile(os.path.join(folder, i)) and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
    if sort:
        res.sort()
    return res


def save_json(obj, file, indent=4, sort_keys=True):
    with open(file, 'w') as f:
        json.dump(obj, f, sort_keys=sort_keys, indent=indent)


ffo.subfiles, ffo.save_json = subfiles, save_json
ffo.__all__ = list(ffo.__all__) + ['subfiles', 'save_json']
from nnunet.dataset_conversion import Task100_MultiTalent as T  # noqa: E402
from nnunet.dataset_conversion.utils import generate_dataset_json  # noqa: E402

GOLDEN = os.path.join(HERE, '..', '..', 'tests', 'golden')
SHAPE = (5, 7, 11)
SLOTS = 1023


def volume(rs, top):
    """Integer labels 0..top as float64, every one of them present."""
    v = rs.randint(0, top + 1, size=SHAPE).astype(np.float64)
    v.ravel()[:top + 1] = np.arange(top + 1)
    return v


def main():
    rs = np.random.RandomState(100)
    arrays, cases = {}, []

    def add(name, vol, labels_in, labels_out, sanity_check=True):
        rec = dict(name=name, labels_in=labels_in, labels_out=labels_out, sanity_check=sanity_check)
        tup = tuple(tuple(i) if isinstance(i, list) else i for i in labels_in)
        arrays[name + '/in'] = vol
        try:
            arrays[name + '/out'] = T.copy_and_convert_segmentation(vol, tup, tuple(labels_out), sanity_check, name)
            rec['raises'] = None
        except RuntimeError as e:
            rec['raises'] = repr(float(e.args[1][0]))                    # the unique the reference met first
        # the mapping itself: every input label 0..1022 once, no sanity check
        arrays[name + '/table'] = T.copy_and_convert_segmentation(np.arange(SLOTS, dtype=np.float64), tup, tuple(labels_out), False, name)
        cases.append(rec)

    add('example', volume(rs, 4), [1, 2, [3, 4], 3], [4, 5, 6, 7])
    add('entry0', volume(rs, 2), [0, 1, 2], [9, 8, 7])
    add('repeated', volume(rs, 3), [1, 1, 2, [2, 3], 1], [10, 11, 12, 13, 14])
    add('to_zero_and_255', volume(rs, 2), [1, 2], [0, 255])
    add('unlisted_no_sanity', volume(rs, 13), [1, 2], [4, 5], False)
    add('unlisted_sanity', volume(rs, 13), [1, [2, 5]], [4, 5], True)
    for t, (li, lo) in T.MultiTalent_task_label_maps.items():
        add(t, volume(rs, len(li)), [int(i) for i in li], [int(i) for i in lo])
    special = volume(rs, 2)
    special.ravel()[20:27] = [-1.0, 1e-21, 1e-20, np.nan, -np.inf, -0.0, -3.5]
    add('legal_specials', special, [1, 2], [4, 5])
    bad = special.copy()
    bad.ravel()[40:46] = [2.5, np.inf, 7.0, 1e30, 70000.0, 0.5]
    add('offenders', bad, [1, 2], [4, 5])
    add('offenders_no_sanity', bad, [1, 2], [4, 5], False)
    np.savez_compressed(os.path.join(GOLDEN, 'dataset_conversion.npz'), **arrays)

    tr = ['003_liver_1_0000.nii.gz', '003_liver_10_0000.nii.gz', '003_liver_2_0000.nii.gz', '009_spleen_7_0000.nii.gz',
          '062_pancreas_0004_0000.nii.gz']
    ts = ['009_spleen_1_0000.nii.gz', '003_liver_77_0000.nii.gz']
    with tempfile.TemporaryDirectory() as d:
        for folder, names in (('imagesTr', tr), ('imagesTs', ts)):
            os.makedirs(os.path.join(d, folder))
            for n in names + ['notes.txt']:
                open(os.path.join(d, folder, n), 'wb').close()
        generate_dataset_json(os.path.join(d, 'dataset.json'), os.path.join(d, 'imagesTr'), os.path.join(d, 'imagesTs'), ("CT",),
                              T.MultiTalent_labels, "Task100_MultiTalent")
        with open(os.path.join(d, 'dataset.json')) as f:
            with_ts = json.load(f)
        generate_dataset_json(os.path.join(d, 'dataset.json'), os.path.join(d, 'imagesTr'), None, ("CT", "MR"), {0: 'background', 1: 'x'},
                              "Other", license="mine", dataset_description="d", dataset_reference="r", dataset_release='1.1')
        with open(os.path.join(d, 'dataset.json')) as f:
            without_ts = json.load(f)
    with open(os.path.join(GOLDEN, 'dataset_conversion.json'), 'w') as f:
        json.dump({'cases': cases, 'imagesTr': tr, 'imagesTs': ts, 'dataset_json': with_ts, 'dataset_json_no_test': without_ts}, f, indent=1)
    print('wrote', len(cases), 'cases')


if __name__ == '__main__':
    main()
