"""Golden `summary.csv` texts for the region-based evaluation: the REAL reference's nnunet/evaluation/region_based_evaluation.py
(`evaluate_regions`, :53-110, with its `evaluate_case` and `create_region_from_mask`), run on CPU in the build container on the
seeded folders of tests/region_cases.py with the KiTS and the BraTS regions.

Substitutions for what this image lacks, at third-party seams:
  * SimpleITK (`sitk.ReadImage`, `sitk.GetArrayFromImage`) -> multitalent_amd/utilities/nifti_io.read_image and its array [z, y, x];
  * `medpy.metric.dc` -> a three-line restatement of medpy's published definition, 2 |A & B| / (|A| + |B|), 0.0 for two empty masks;
  * batchgenerators' `subfiles` / `join` -> os.listdir / os.path.join (tools/oracle_gen/ref_import.py).
The reference's worker pool runs as it is (forked workers inherit the substitutions).

Writes the two csv texts to tests/golden/region_evaluation.json; the test rebuilds the folders.
Run: python tools/oracle_gen/make_golden_region_evaluation.py"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ref_import
ref_import.install()

import region_cases as RC
from multitalent_amd.utilities import nifti_io
nifti_io._have_sitk = lambda: False                  # ref_import's empty stand-in module is not SimpleITK: nifti_io's own reader / writer

import batchgenerators.utilities.file_and_folder_operations as ffo


def _subfiles(folder, join=True, prefix=None, suffix=None, sort=True):
    res = [os.path.join(folder, i) if join else i for i in os.listdir(folder)
           if os.path.isfile(os.path.join(folder, i)) and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
    return sorted(res) if sort else res


ffo.subfiles = _subfiles
ffo.__all__ = list(ffo.__all__) + ['subfiles']

import SimpleITK as sitk
sitk.ReadImage = lambda fname: nifti_io.read_image(fname)
sitk.GetArrayFromImage = lambda img: np.asarray(img.array)


def _dc(result, reference):
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    size = np.count_nonzero(result) + np.count_nonzero(reference)
    return 2. * np.count_nonzero(result & reference) / float(size) if size else 0.0


import medpy
medpy.metric = types.ModuleType('medpy.metric')
medpy.metric.dc = _dc
sys.modules['medpy.metric'] = medpy.metric

import nnunet.evaluation.region_based_evaluation as ref_regions


def main():
    out = {'shape': list(RC.SHAPE), 'cases': RC.CASES}
    for key, regions in (('kits', ref_regions.get_KiTS_regions()), ('brats', ref_regions.get_brats_regions())):
        with tempfile.TemporaryDirectory() as d:
            pred, gt = os.path.join(d, 'pred'), os.path.join(d, 'gt')
            os.makedirs(pred)
            os.makedirs(gt)
            RC.write_folders(pred, gt)
            ref_regions.evaluate_regions(pred, gt, regions, processes=2)
            with open(os.path.join(pred, 'summary.csv')) as f:
                out[key] = {'regions': {k: list(v) for k, v in regions.items()}, 'summary_csv': f.read()}
        print(out[key]['summary_csv'])
    dst = os.path.join(ROOT, 'tests', 'golden', 'region_evaluation.json')
    with open(dst, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
