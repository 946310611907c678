"""Host logic of the stock prediction / ensembling drivers (no GPU): the folder-scan assertions of `merge`, the
`regions_class_order` consistency assertion, the dtype / shape / member-count rejections (all raised before any device call),
`predict_simple` argument parsing and model-folder resolution, the refused modes, `collect_cv_niftis` on a missing fold."""
import os
import pickle

import numpy as np
import pytest


def props(shape, order=None):
    p = dict(size_after_cropping=np.array(shape), original_size_of_raw_data=np.array([s + 2 for s in shape]),
             crop_bbox=[[1, 1 + s] for s in shape], itk_spacing=(1., 1., 1.), itk_origin=(0., 0., 0.), itk_direction=tuple(np.eye(3).ravel()))
    if order is not None:
        p['regions_class_order'] = order
    return p


def write_member(folder, name, arr, p):
    os.makedirs(folder, exist_ok=True)
    np.savez_compressed(os.path.join(folder, name + '.npz'), softmax=arr)
    with open(os.path.join(folder, name + '.pkl'), 'wb') as f:
        pickle.dump(p, f)
    return os.path.join(folder, name + '.npz'), os.path.join(folder, name + '.pkl')


@pytest.fixture(autouse=True)
def no_device_call(monkeypatch):
    """every rejection here comes before the device is asked"""
    import multitalent_amd.inference.ensemble_predictions as ep

    def boom(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(ep, 'merge_on_device', boom)
    monkeypatch.setattr(ep, 'ensemble_classify', boom)


def test_merge_folder_scan_assertions(tmp_path):
    from multitalent_amd.inference.ensemble_predictions import merge
    shape = (2, 3, 4)
    a = np.zeros((2,) + shape, np.float16)
    f0, f1 = str(tmp_path / 'f0'), str(tmp_path / 'f1')
    write_member(f0, 'c0', a, props(shape)); write_member(f0, 'c1', a, props(shape))
    write_member(f1, 'c0', a, props(shape))
    with pytest.raises(AssertionError, match="Not all patient npz are available in all folders"):
        merge([f0, f1], str(tmp_path / 'out'), 2)
    np.savez_compressed(os.path.join(f1, 'c1.npz'), softmax=a)
    with pytest.raises(AssertionError, match="Not all patient pkl are available in all folders"):
        merge([f0, f1], str(tmp_path / 'out'), 2)
    assert os.path.isdir(str(tmp_path / 'out'))
    with pytest.raises(AssertionError, match="Not all patient pkl"):
        merge([f0, f1], str(tmp_path / 'out_pp'), 2, postprocessing_file=str(tmp_path / 'pp.json'))
    assert os.path.isdir(str(tmp_path / 'out_pp' / 'not_postprocessed'))


def test_regions_class_order_must_agree(tmp_path):
    from multitalent_amd.inference.ensemble_predictions import merge_files
    shape = (2, 3, 4)
    a = np.zeros((2,) + shape, np.float16)
    m0 = write_member(str(tmp_path / 'f0'), 'c', a, props(shape, [1, 2]))
    m1 = write_member(str(tmp_path / 'f1'), 'c', a, props(shape, [2, 1]))
    m2 = write_member(str(tmp_path / 'f2'), 'c', a, props(shape))
    for other in (m1, m2):
        with pytest.raises(AssertionError, match="regions_class_orders of all files must be the same"):
            merge_files([m0[0], other[0]], [m0[1], other[1]], str(tmp_path / 'o.nii.gz'), True, False)
    with pytest.raises(AssertionError, match="regions_class_orders of all files must be the same"):
        merge_files([m2[0], m0[0]], [m2[1], m0[1]], str(tmp_path / 'o.nii.gz'), True, False)


def test_member_rejections(tmp_path):
    from multitalent_amd.inference.ensemble_predictions import MAX_MEMBERS, merge_files
    shape = (2, 3, 4)
    ok = write_member(str(tmp_path / 'ok'), 'c', np.zeros((2,) + shape, np.float16), props(shape))
    f32 = write_member(str(tmp_path / 'f32'), 'c', np.zeros((2,) + shape, np.float32), props(shape))
    with pytest.raises(TypeError, match=os.path.join('f32', 'c.npz')):
        merge_files([ok[0], f32[0]], [ok[1], f32[1]], str(tmp_path / 'o.nii.gz'), True, False)
    low = write_member(str(tmp_path / 'low'), 'c', np.zeros((2, 2, 2, 4), np.float16), props(shape))
    with pytest.raises(NotImplementedError, match=os.path.join('low', 'c.npz')):
        merge_files([ok[0], low[0]], [ok[1], low[1]], str(tmp_path / 'o.nii.gz'), True, False)
    chan = write_member(str(tmp_path / 'chan'), 'c', np.zeros((3,) + shape, np.float16), props(shape))
    with pytest.raises(NotImplementedError):
        merge_files([ok[0], chan[0]], [ok[1], chan[1]], str(tmp_path / 'o.nii.gz'), True, False)
    assert MAX_MEMBERS == 16
    with pytest.raises(ValueError, match="at most 16 members"):
        merge_files([ok[0]] * 17, [ok[1]] * 17, str(tmp_path / 'o.nii.gz'), True, False)
    # an existing output is kept when override is off: nothing is even read
    open(str(tmp_path / 'o.nii.gz'), 'w').close()
    merge_files([str(tmp_path / 'missing.npz')], [str(tmp_path / 'missing.pkl')], str(tmp_path / 'o.nii.gz'), False, False)


def test_max_members_is_the_headers():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, 'include', 'mtseg.h')).read()
    from multitalent_amd.inference.ensemble_predictions import MAX_MEMBERS
    assert int(re.search(r'#define MT_ENSEMBLE_MAX_MEMBERS\s+(\d+)', txt).group(1)) == MAX_MEMBERS


def test_predict_simple_arguments_and_model_folder(tmp_path, monkeypatch):
    from multitalent_amd.inference import predict_simple as ps
    a = ps.build_parser().parse_args(['-i', 'in', '-o', 'out', '-t', 'Task555_Tiny'])
    assert (a.trainer_class_name, a.cascade_trainer_class_name, a.model, a.plans_identifier) == \
        ('nnUNetTrainerV2', 'nnUNetTrainerV2CascadeFullRes', '3d_fullres', 'nnUNetPlansv2.1')
    assert (a.folds, a.save_npz, a.lowres_segmentations, a.part_id, a.num_parts) == ('None', False, 'None', 0, 1)
    assert (a.num_threads_preprocessing, a.num_threads_nifti_save, a.disable_tta, a.overwrite_existing) == (6, 2, False, False)
    assert (a.mode, a.all_in_gpu, a.step_size, a.chk, a.disable_mixed_precision) == ('normal', 'None', 0.5, 'model_final_checkpoint', False)
    a = ps.build_parser().parse_args(['-i', 'in', '-o', 'out', '-t', '555', '-tr', 'T', '-ctr', 'CT', '-m', '3d_lowres', '-p', 'P', '-f', '0', '3',
                                      '-z', '-l', 'low', '--part_id', '1', '--num_parts', '2', '--num_threads_preprocessing', '1',
                                      '--num_threads_nifti_save', '1', '--disable_tta', '--overwrite_existing', '--mode', 'fast',
                                      '--all_in_gpu', 'True', '--step_size', '0.7', '-chk', 'model_best', '--disable_mixed_precision'])
    assert (a.task_name, a.folds, a.save_npz, a.part_id, a.num_parts, a.mode, a.chk) == ('555', ['0', '3'], True, 1, 2, 'fast', 'model_best')
    assert ps.parse_folds(['0', '3']) == [0, 3] and ps.parse_folds(['all']) == ['all'] and ps.parse_folds('None') is None
    with pytest.raises(ValueError):
        ps.parse_folds('0')
    # model folder: <RESULTS_FOLDER>/nnUNet/<model>/<task>/<trainer>__<plans>; a task id goes through the preprocessed root
    res, pre = tmp_path / 'res', tmp_path / 'pre'
    folder = res / 'nnUNet' / '3d_fullres' / 'Task555_Tiny' / 'nnUNetTrainerV2__nnUNetPlansv2.1'
    folder.mkdir(parents=True)
    (pre / 'Task555_Tiny').mkdir(parents=True)
    monkeypatch.setenv('RESULTS_FOLDER', str(res))
    monkeypatch.setenv('nnUNet_preprocessed', str(pre))
    assert ps.model_folder('3d_fullres', 'Task555_Tiny', 'nnUNetTrainerV2', 'nnUNetPlansv2.1') == str(folder)
    assert ps.model_folder('3d_fullres', '555', 'nnUNetTrainerV2', 'nnUNetPlansv2.1') == str(folder)
    with pytest.raises(AssertionError, match="model output folder not found"):
        ps.model_folder('3d_lowres', 'Task555_Tiny', 'nnUNetTrainerV2', 'nnUNetPlansv2.1')
    for m in ('2d', '3d_cascade_fullres'):
        with pytest.raises(NotImplementedError, match=m):
            ps.model_folder(m, 'Task555_Tiny', 'nnUNetTrainerV2', 'nnUNetPlansv2.1')
        with pytest.raises(NotImplementedError, match=m):
            ps.main(['-i', 'in', '-o', 'out', '-t', 'Task555_Tiny', '-m', m])
    with pytest.raises(AssertionError, match="-m must be"):
        ps.model_folder('4d', 'Task555_Tiny', 'nnUNetTrainerV2', 'nnUNetPlansv2.1')


def test_refused_modes_and_cascade_inputs(tmp_path):
    from multitalent_amd.inference.predict import check_input_folder_and_return_caseIDs, predict_cases, predict_from_folder
    from multitalent_amd.inference import predict_MultiTalent
    assert check_input_folder_and_return_caseIDs is predict_MultiTalent.check_input_folder_and_return_caseIDs     # imported, not copied
    for mode in ('fast', 'fastest'):
        with pytest.raises(ValueError, match=mode):
            predict_from_folder(str(tmp_path), str(tmp_path), str(tmp_path / 'o'), None, False, 1, 1, None, 0, 1, True, mode=mode)
    with pytest.raises(ValueError, match="unrecognized mode"):
        predict_from_folder(str(tmp_path), str(tmp_path), str(tmp_path / 'o'), None, False, 1, 1, None, 0, 1, True, mode='slow')
    assert not os.path.exists(str(tmp_path / 'o'))
    with pytest.raises(NotImplementedError, match="lowres_segmentations"):
        predict_from_folder(str(tmp_path), str(tmp_path), str(tmp_path / 'o'), None, False, 1, 1, str(tmp_path), 0, 1, True)
    with pytest.raises(NotImplementedError, match="segs_from_prev_stage"):
        predict_cases(str(tmp_path), [['a_0000.nii.gz']], ['a.nii.gz'], None, False, 1, 1, segs_from_prev_stage=['s.nii.gz'])


def test_collect_cv_niftis_missing_fold(tmp_path):
    from multitalent_amd.postprocessing.consolidate_postprocessing import collect_cv_niftis, consolidate_folds
    for f in (0, 2):
        os.makedirs(str(tmp_path / ('fold_%d' % f) / 'validation_raw'))
        open(str(tmp_path / ('fold_%d' % f) / 'validation_raw' / ('case%d.nii.gz' % f)), 'w').close()
    with pytest.raises(RuntimeError, match=r"some folds are missing.*\[1\]"):
        collect_cv_niftis(str(tmp_path), str(tmp_path / 'cv_niftis_raw'), folds=(0, 1, 2))
    assert not os.path.exists(str(tmp_path / 'cv_niftis_raw'))
    collect_cv_niftis(str(tmp_path), str(tmp_path / 'cv_niftis_raw'), folds=(0, 2))
    assert sorted(os.listdir(str(tmp_path / 'cv_niftis_raw'))) == ['case0.nii.gz', 'case2.nii.gz']
    # the number of collected masks must equal the number of ground-truth files
    os.makedirs(str(tmp_path / 'gt_niftis'))
    with pytest.raises(AssertionError, match="trained all the folds"):
        consolidate_folds(str(tmp_path), folds=(0, 2))
