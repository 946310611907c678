"""`nnUNet_plan_and_preprocess` end to end on the device: a toy task of five CT cases (planning_cases.TASK901: different shapes
around 40x44x18 with the coarse axis last, an all-zero margin around every case, labels 0..2, one label file stored as float and
one as uint8) goes from raw NIfTI files to plans and preprocessed cases.  The plan is the reference's (tests/golden/planning.json);
the preprocessed cases are bit-identical to ImageCropper, DatasetAnalyzer and GenericPreprocessor.run called by hand, which have
their own tests against the reference: this file pins the wiring.  Also the device half of verify_dataset_integrity."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planning_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
PLANS = 'nnUNetPlansv2.1_plans_3D.pkl'
DATA = 'nnUNetData_plans_v2.1'
ARGS = ('-pl3d', 'ExperimentPlanner3D_v21', '--verify_dataset_integrity')


@pytest.fixture(scope='module')
def env(dev, tmp_path_factory):
    e = PC.ToyEnvironment(tmp_path_factory.mktemp('plan_and_preprocess'))
    e.plan_and_preprocess(PC.TASK901, *ARGS)
    e.task = PC.TASK901['name']
    e.cropped_task, e.out = os.path.join(e.cropped, e.task), os.path.join(e.preprocessed, e.task)
    e.plans = PC.load_pickle(os.path.join(e.out, PLANS))
    yield e
    e.close()


def _get(node, key):
    return next(v for k, v in node['dict'] if k == key)


def test_the_plan_is_the_references(env):
    gold = _get(_get(_get(_get(_get(PC.load_golden(), 'fingerprints'), 'tiny'), 'planners'), 'ExperimentPlanner3D_v21'), 'plans')
    plans = PC.load_pickle(os.path.join(env.out, PLANS))
    ip = plans['dataset_properties']['intensityproperties']             # from the device; DatasetAnalyzer's tests pin its values
    assert list(ip.keys()) == [0] and ip[0]['sd'] > 0 and len(ip[0]['local_props']) == 5
    plans['dataset_properties']['intensityproperties'] = None
    fp = PC.toy_fingerprint(PC.TASK901)
    assert PC.encode(PC.compact_plans(PC.relativize(plans, {env.cropped_task: '<cropped>', env.out: '<preprocessed>'}), fp)) == gold
    assert gold == PC.encode(PC.decode(gold)) and dict(gold['dict'])['dataset_properties'] == '<fingerprint>'
    assert plans['transpose_forward'] == [2, 0, 1]                      # the coarse axis is last in the files
    for f in ('dataset_properties.pkl', 'dataset.json'):
        assert os.path.isfile(os.path.join(env.out, f))
    assert sorted(os.listdir(os.path.join(env.out, 'gt_segmentations'))) == [c['id'] + '.nii.gz' for c in PC.TASK901['cases']]
    for c in PC.TASK901['cases']:
        props = PC.load_pickle(os.path.join(env.cropped_task, c['id'] + '.pkl'))
        assert dict(props['use_nonzero_mask_for_norm']) == {0: False}
        assert tuple(props['size_after_cropping']) == PC.body_shape(c) != tuple(c['shape'])        # the crop changed the shape


def test_stage0_equals_the_stages_called_by_hand(env, tmp_path):
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer
    from multitalent_amd.experiment_planning.utils import create_lists_from_splitted_dataset
    from multitalent_amd.preprocessing.device_cropping import ImageCropper
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    plans = env.plans
    raw = os.path.join(env.raw, env.task)
    cropped, out = str(tmp_path / 'cropped'), str(tmp_path / 'out')
    ImageCropper(2, cropped).run_cropping(create_lists_from_splitted_dataset(raw)[0], overwrite_existing=False)
    shutil.copy(os.path.join(raw, 'dataset.json'), cropped)
    dp = DatasetAnalyzer(cropped, overwrite=True, num_processes=2).analyze_dataset(True)
    assert PC.encode(dp) == PC.encode(plans['dataset_properties'])
    PC.assert_same_cases(PC.load_cases(env.cropped_task), PC.load_cases(cropped), ignore=('use_nonzero_mask_for_norm',))
    target = plans['plans_per_stage'][0]['current_spacing']
    pre = GenericPreprocessor(plans['normalization_schemes'], plans['use_mask_for_norm'], plans['transpose_forward'],
                              dp['intensityproperties'])
    pre.run([target], cropped, out, DATA, 2)
    got, want = PC.load_cases(os.path.join(env.out, DATA + '_stage0')), PC.load_cases(os.path.join(out, DATA + '_stage0'))
    assert len(got) == 5
    PC.assert_same_cases(got, want, ignore=('use_nonzero_mask_for_norm',))
    for k, (a, props) in got.items():
        assert dict(props['use_nonzero_mask_for_norm']) == {0: False}
        assert a.dtype == np.float32 and a.shape == (2,) + PC.expected_shape(props, target, plans['transpose_forward'])
        assert a.shape[1] < a.shape[2] and set(np.unique(a[-1])) <= {-1.0, 0.0, 1.0, 2.0}
        assert sorted(props['class_locations']) == [1, 2] and all(len(v) > 0 for v in props['class_locations'].values())


def test_a_second_run_crops_nothing_again_and_gives_the_same_files(env):
    stage = os.path.join(env.out, DATA + '_stage0')
    before = PC.load_cases(stage)
    stamps = {f: os.stat(os.path.join(env.cropped_task, f)).st_mtime_ns for f in os.listdir(env.cropped_task) if f.endswith('.npz')}
    plans = PC.load_pickle(os.path.join(env.out, PLANS))
    env.plan_and_preprocess(PC.TASK901, *ARGS)
    assert stamps == {f: os.stat(os.path.join(env.cropped_task, f)).st_mtime_ns for f in stamps}
    assert PC.encode(PC.load_pickle(os.path.join(env.out, PLANS))) == PC.encode(plans)
    PC.assert_same_cases(PC.load_cases(stage), before)


def _planted(env, tmp_path, case, plant, image=False):
    from multitalent_amd.utilities.nifti_io import read_image, write_image
    folder = str(tmp_path / env.task)
    shutil.copytree(os.path.join(env.raw, env.task), folder)
    f = os.path.join(folder, 'imagesTr', case + '_0000.nii.gz') if image else os.path.join(folder, 'labelsTr', case + '.nii.gz')
    img = read_image(f)
    write_image(plant(np.array(img.array)), f, img.spacing, img.origin, img.direction)
    return folder, f


def test_integrity_check_finds_an_undeclared_label(env, tmp_path, capsys):
    from multitalent_amd.preprocessing.sanity_checks import verify_dataset_integrity
    def plant(a):
        a[5, 6, 7] = 7
        return a
    folder, f = _planted(env, tmp_path, 'tiny_002', plant)
    with pytest.raises(AssertionError, match=r"Found unexpected labels in the training dataset(.|\n)*tiny_002\.nii\.gz: \[7\]"):
        verify_dataset_integrity(folder)
    assert "Unexpected labels found in file %s" % f in capsys.readouterr().out


def test_integrity_check_finds_a_fractional_label(env, tmp_path, capsys):
    from multitalent_amd.preprocessing.sanity_checks import verify_dataset_integrity
    def plant(a):
        a = a.astype(np.float32)
        a[5, 6, 7] = 0.5
        return a
    folder, f = _planted(env, tmp_path, 'tiny_003', plant)
    with pytest.raises(AssertionError, match=r"tiny_003\.nii\.gz: \[(np\.float32\()?0\.5\)?\]"):
        verify_dataset_integrity(folder)
    assert "Unexpected labels found in file %s" % f in capsys.readouterr().out


def test_integrity_check_only_prints_a_nan_in_an_image(env, tmp_path, capsys):
    from multitalent_amd.preprocessing.sanity_checks import verify_dataset_integrity
    def plant(a):
        a[9, 9, 9] = np.nan
        return a
    folder, f = _planted(env, tmp_path, 'tiny_001', plant, image=True)
    verify_dataset_integrity(folder)
    out = capsys.readouterr().out
    assert "There are NAN values in image %s" % f in out and "Some images have nan values in them" in out and "Dataset OK" in out


def test_two_stages_through_run_preprocessing(env, tmp_path, capsys):
    """A hand-edited copy of the tiny plan with a second, coarser stage in front: both stage folders, shapes by each spacing;
    `num_threads` as a number and as (low resolution, full resolution)."""
    import copy
    import pickle
    from multitalent_amd.experiment_planning.experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21
    out = str(tmp_path / 'out')
    os.makedirs(out)
    plans = copy.deepcopy(env.plans)
    full = plans['plans_per_stage'][0]
    coarse = copy.deepcopy(full)
    coarse['current_spacing'] = full['current_spacing'] * np.array([1.0, 2.0, 2.0])
    plans['plans_per_stage'] = {0: coarse, 1: full}
    plans['num_stages'] = 2
    planner = ExperimentPlanner3D_v21(env.cropped_task, out)
    with open(planner.plans_fname, 'wb') as f:
        pickle.dump(plans, f)
    planner.load_my_plans()
    for num_threads in (2, (1, 2)):
        planner.run_preprocessing(num_threads)
        for stage in (0, 1):
            cases = PC.load_cases(os.path.join(out, DATA + '_stage%d' % stage))
            assert len(cases) == 5
            for k, (a, props) in cases.items():
                want = PC.expected_shape(props, plans['plans_per_stage'][stage]['current_spacing'], plans['transpose_forward'])
                assert a.shape[1:] == want and tuple(props['size_after_resampling']) == want, (stage, k)
        shutil.rmtree(os.path.join(out, DATA + '_stage0'))
        shutil.rmtree(os.path.join(out, DATA + '_stage1'))
    assert sorted(os.listdir(os.path.join(out, 'gt_segmentations'))) == [c['id'] + '.nii.gz' for c in PC.TASK901['cases']]
