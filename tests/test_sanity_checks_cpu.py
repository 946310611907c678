"""The host half of `verify_dataset_integrity` (`verify_dataset_structure`: files, dataset.json, geometry headers) on tiny NIfTI
folders, one case per outcome of the reference (preprocessing/sanity_checks.py:45-247).  No device is needed; the voxel half has
its tests in test_plan_and_preprocess_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

from multitalent_amd.preprocessing import sanity_checks as SC
from multitalent_amd.utilities.nifti_io import write_image

SHAPE = (5, 6, 7)
GEO = dict(spacing=(0.75, 0.75, 3.0), origin=(-10.0, 20.0, 5.5))


def _task(tmp_path, cases=('a_001', 'a_002'), modalities=1, labels=(0, 1, 2), test=(), name='Task777_Check'):
    folder = tmp_path / name
    for sub in ('imagesTr', 'labelsTr', 'imagesTs'):
        os.makedirs(folder / sub)
    rs = np.random.RandomState(3)
    for c in cases:
        for m in range(modalities):
            write_image(rs.rand(*SHAPE).astype(np.float32), str(folder / 'imagesTr' / ('%s_%04d.nii.gz' % (c, m))), **GEO)
        write_image(rs.randint(0, 3, SHAPE).astype(np.uint8), str(folder / 'labelsTr' / (c + '.nii.gz')), **GEO)
    for c in test:
        for m in range(modalities):
            write_image(rs.rand(*SHAPE).astype(np.float32), str(folder / 'imagesTs' / ('%s_%04d.nii.gz' % (c, m))), **GEO)
    d = {'modality': {str(m): 'CT' for m in range(modalities)}, 'labels': {str(i): 'l%d' % i for i in labels},
         'training': [{'image': './imagesTr/%s.nii.gz' % c, 'label': './labelsTr/%s.nii.gz' % c} for c in cases],
         'test': ['./imagesTs/%s.nii.gz' % c for c in test]}
    with open(folder / 'dataset.json', 'w') as f:
        json.dump(d, f)
    return folder


def _rewrite_json(folder, **changes):
    with open(folder / 'dataset.json') as f:
        d = json.load(f)
    d.update(changes)
    with open(folder / 'dataset.json', 'w') as f:
        json.dump(d, f)


def test_clean_folder_passes(tmp_path, capsys):
    SC.verify_dataset_structure(str(_task(tmp_path, modalities=2)))
    out = capsys.readouterr().out
    assert "Dataset OK" in out and "WARNING" not in out


def test_missing_modality(tmp_path):
    folder = _task(tmp_path, modalities=2)
    os.remove(folder / 'imagesTr' / 'a_002_0001.nii.gz')
    with pytest.raises(AssertionError, match="some image files are missing for case a_002"):
        SC.verify_dataset_structure(str(folder))


def test_missing_label_file(tmp_path):
    folder = _task(tmp_path)
    os.remove(folder / 'labelsTr' / 'a_001.nii.gz')
    with pytest.raises(AssertionError, match="could not find label file for case a_001"):
        SC.verify_dataset_structure(str(folder))


def test_straggler(tmp_path):
    folder = _task(tmp_path)
    write_image(np.zeros(SHAPE, np.float32), str(folder / 'imagesTr' / 'zz_009_0000.nii.gz'), **GEO)
    with pytest.raises(AssertionError, match=r"training cases in imagesTr that are not listed in dataset.json: \['zz_009_0000.nii.gz'\]"):
        SC.verify_dataset_structure(str(folder))
    os.remove(folder / 'imagesTr' / 'zz_009_0000.nii.gz')
    write_image(np.zeros(SHAPE, np.uint8), str(folder / 'labelsTr' / 'zz_009.nii.gz'), **GEO)
    with pytest.raises(AssertionError, match="training cases in labelsTr that are not listed"):
        SC.verify_dataset_structure(str(folder))


def test_duplicate_case(tmp_path):
    folder = _task(tmp_path)
    with open(folder / 'dataset.json') as f:
        tr = json.load(f)['training']
    _rewrite_json(folder, training=tr + tr[:1])
    with pytest.raises(RuntimeError, match="found duplicate training cases in dataset.json"):
        SC.verify_dataset_structure(str(folder))


def test_non_consecutive_labels(tmp_path):
    with pytest.raises(AssertionError, match=r"Labels must be in consecutive order .* The labels \[3\] do not satisfy"):
        SC.verify_dataset_structure(str(_task(tmp_path, labels=(0, 1, 3))))
    with pytest.raises(AssertionError, match="The first label must be 0"):
        SC.verify_dataset_structure(str(_task(tmp_path / 'b', labels=(1, 2))))


def _reorigin(folder, case, origin):
    write_image(np.ones(SHAPE, np.float32), str(folder / 'imagesTr' / (case + '_0000.nii.gz')), spacing=GEO['spacing'], origin=origin)


def test_origin_beyond_the_tolerance_warns_at_the_end(tmp_path, capsys):
    folder = _task(tmp_path)
    _reorigin(folder, 'a_002', (-10.0, 20.5, 5.5))                 # |20.5 - 20| > 1e-3 + 1e-3 * 20
    with pytest.raises(Warning, match="GEOMETRY MISMATCH FOUND"):
        SC.verify_dataset_structure(str(folder))
    out = capsys.readouterr().out
    assert "the origin does not match between the images:" in out and "a_002" in out


def test_origin_within_the_tolerance_passes(tmp_path, capsys):
    folder = _task(tmp_path)
    _reorigin(folder, 'a_002', (-10.0, 20.015, 5.5))               # 0.015 < 1e-3 + 1e-3 * 20 = 0.021
    SC.verify_dataset_structure(str(folder))
    assert "Dataset OK" in capsys.readouterr().out


def test_differing_spacing_warns(tmp_path, capsys):
    folder = _task(tmp_path)
    write_image(np.ones(SHAPE, np.float32), str(folder / 'imagesTr' / 'a_001_0000.nii.gz'), spacing=(0.75, 0.76, 3.0), origin=GEO['origin'])
    with pytest.raises(Warning, match="GEOMETRY MISMATCH FOUND"):
        SC.verify_dataset_structure(str(folder))
    assert "the spacing does not match between the images" in capsys.readouterr().out


def test_clean_test_set_and_missing_test_file(tmp_path, capsys):
    folder = _task(tmp_path, modalities=2, test=('t_001', 't_002'))
    SC.verify_dataset_structure(str(folder))
    assert "Verifying test set" in capsys.readouterr().out
    os.remove(folder / 'imagesTs' / 't_002_0001.nii.gz')
    with pytest.raises(AssertionError, match="some image files are missing for case t_002"):
        SC.verify_dataset_structure(str(folder))


def test_axis_codes_follow_the_affine(tmp_path, capsys):
    assert SC.axis_codes((1, 0, 0, 0, 1, 0, 0, 0, 1)) == ('L', 'P', 'S')           # ITK's identity is LPS
    assert SC.axis_codes((-1, 0, 0, 0, -1, 0, 0, 0, 1)) == ('R', 'A', 'S')
    assert SC.axis_codes((0, 0, 1, 1, 0, 0, 0, -1, 0)) == ('P', 'I', 'L')
    c, s = np.cos(0.3), np.sin(0.3)
    assert SC.axis_codes((c, -s, 0, s, c, 0, 0, 0, 1)) == ('L', 'P', 'S')           # a small rotation keeps the codes
    folder = _task(tmp_path)
    write_image(np.ones(SHAPE, np.float32), str(folder / 'imagesTr' / 'a_001_0000.nii.gz'), direction=(-1, 0, 0, 0, -1, 0, 0, 0, 1), **GEO)
    with pytest.raises(Warning):                                                    # the flipped direction is a geometry mismatch too
        SC.verify_dataset_structure(str(folder))
    assert "WARNING: Not all images in the dataset have the same axis ordering" in capsys.readouterr().out


def test_the_voxel_pass_has_no_cpu_fallback(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        SC.verify_dataset_integrity(str(_task(tmp_path)))
