"""Shared by tests/test_region_evaluation_gpu.py and tools/oracle_gen/make_golden_region_evaluation.py (not a test module): the
seeded label volumes behind tests/golden/region_evaluation.json and the writer of the two folders.

Four predicted cases of shape (24, 40, 48) with labels 0..3 (one ellipsoid per label, the ground truth's shifted and rescaled, a
little label noise on both), and a fifth ground truth without prediction:
  case_00, case_03   every label in both volumes;
  case_01            labels 2 and 3 in neither volume: KiTS' "tumor" and BraTS' "tumor core" / "enhancing tumor" are NaN;
  case_02            labels 2 and 3 missing from the prediction only: those regions score 0.0;
  case_04            ground truth only: the "not predicted" warning."""
import os

import numpy as np

from evaluation_cases import ellipsoid

SHAPE = (24, 40, 48)
SPACING_XYZ = (0.75, 1.25, 3.0)
CASES = [dict(name='case_00', seed=21, pred_labels=(1, 2, 3), gt_labels=(1, 2, 3)),
         dict(name='case_01', seed=22, pred_labels=(1,), gt_labels=(1,)),
         dict(name='case_02', seed=23, pred_labels=(1,), gt_labels=(1, 2, 3)),
         dict(name='case_03', seed=24, pred_labels=(1, 2, 3), gt_labels=(1, 2, 3)),
         dict(name='case_04', seed=25, pred_labels=None, gt_labels=(1, 2, 3))]


def region_case(seed, pred_labels, gt_labels):
    """-> (prediction or None, ground truth): uint8 label volumes of SHAPE"""
    rng = np.random.default_rng(seed)
    s = np.array(SHAPE, dtype=np.float64)
    pred, gt = np.zeros(SHAPE, np.uint8), np.zeros(SHAPE, np.uint8)
    anchors = ((0.3, 0.3, 0.3), (0.65, 0.6, 0.4), (0.4, 0.55, 0.75))
    for lab, a in zip((1, 2, 3), anchors):
        c = (np.array(a) + rng.uniform(-0.04, 0.04, 3)) * s
        r = rng.uniform(0.12, 0.2, 3) * s
        shift = rng.uniform(-2.0, 2.0, 3)
        scale = rng.uniform(0.85, 1.15, 3)
        if pred_labels is not None and lab in pred_labels:
            pred[ellipsoid(SHAPE, c, r)] = lab
        if lab in gt_labels:
            gt[ellipsoid(SHAPE, c + shift, r * scale)] = lab
    for vol, labels in ((pred, pred_labels), (gt, gt_labels)):          # a few stray voxels of the labels the volume has
        if labels:
            stray = rng.random(SHAPE) < 0.002
            vol[stray] = rng.choice(np.array(labels, dtype=np.uint8), int(stray.sum()))
    return (pred if pred_labels is not None else None), gt


def write_folders(folder_pred, folder_gt):
    """Writes the cases as .nii.gz; -> the names of the predicted cases, sorted."""
    from multitalent_amd.utilities import nifti_io
    names = []
    for c in CASES:
        pred, gt = region_case(c['seed'], c['pred_labels'], c['gt_labels'])
        nifti_io.write_image(gt, os.path.join(folder_gt, c['name'] + '.nii.gz'), SPACING_XYZ)
        if pred is not None:
            nifti_io.write_image(pred, os.path.join(folder_pred, c['name'] + '.nii.gz'), SPACING_XYZ)
            names.append(c['name'])
    return sorted(names)
