"""Experiment planning against the reference (no device): tests/golden/planning.json holds what the reference's planners,
`get_pool_and_conv_props*` and `compute_approx_vram_consumption` give (tools/oracle_gen/make_golden_planning.py).  Everything is
compared for EQUALITY in the codec of planning_cases.py: structure, integers, lists, array dtypes and every float bit for bit.
The restatement makes the reference's float64 numpy calls in the reference's order; a differing float is a differing restatement."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planning_cases as PC  # noqa: E402

from multitalent_amd.experiment_planning import common_utils  # noqa: E402
from multitalent_amd.experiment_planning import nnUNet_plan_and_preprocess as driver  # noqa: E402
from multitalent_amd.experiment_planning.alternative_experiment_planning.experiment_planner_pretrained import \
    ExperimentPlanner3D_v21_Pretrained  # noqa: E402
from multitalent_amd.experiment_planning.experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21  # noqa: E402
from multitalent_amd.network_architecture.generic_UNet import Generic_UNet  # noqa: E402
from multitalent_amd.network_architecture.generic_modular_residual_UNet import FabiansUNet  # noqa: E402

PLANNERS = ('ExperimentPlanner', 'ExperimentPlanner3D_v21', 'ExperimentPlanner3D_v21_MultiTalent',
            'ExperimentPlanner3DFabiansResUNet_v21')
FINGERPRINTS = ('ct_large', 'ct_small', 'aniso', 'brain4', 'last_axis', 'tiny')


@pytest.fixture(scope='module')
def gold():
    return PC.load_golden()


def _get(node, key):
    """Member `key` of an encoded dict."""
    for k, v in node['dict']:
        if k == key:
            return v
    raise KeyError(key)


def _plan(planner_name, fp, tmp_path, extra=()):
    cropped, out = str(tmp_path / 'cropped'), str(tmp_path / 'preprocessed')
    os.makedirs(out)
    PC.write_fingerprint_folder(cropped, fp)
    planner = driver._find_planner(planner_name)(cropped, out, *extra)
    planner.plan_experiment()
    return planner, {cropped: '<cropped>', out: '<preprocessed>'}


def _stages(plans):
    st = plans['plans_per_stage']
    return [st[k] for k in sorted(st)]


@pytest.mark.parametrize('fingerprint,planner_name', [(f, p) for f in FINGERPRINTS for p in PLANNERS if f != 'tiny'] +
                         [('tiny', 'ExperimentPlanner3D_v21')])
def test_plans_equal_the_reference(gold, fingerprint, planner_name, tmp_path, capsys):
    rec = _get(_get(gold, 'fingerprints'), fingerprint)
    fp = PC.fingerprint_of(rec)
    want = _get(_get(rec, 'planners'), planner_name)
    planner, roots = _plan(planner_name, fp, tmp_path)
    capsys.readouterr()
    assert os.path.basename(planner.plans_fname) == _get(want, 'fname')
    with open(planner.plans_fname, 'rb') as f:
        plans = pickle.load(f)
    got, ref = PC.encode(PC.compact_plans(PC.relativize(plans, roots), fp)), _get(want, 'plans')
    assert [k for k, _ in got['dict']] == [k for k, _ in ref['dict']]
    for (k, a), (_, b) in zip(got['dict'], ref['dict']):
        assert a == b, "plans[%r] differs from the reference's" % k
    assert got == ref
    assert dict(got['dict'])['dataset_properties'] == '<fingerprint>' and dict(got['dict'])['list_of_npz_files'] == '<fingerprint>'
    assert PC.encode(PC.case_mask(next(iter(roots)), fp['cases'])) == _get(want, 'case_mask')


def test_the_fingerprints_cover_what_they_were_chosen_for(gold):
    """The golden file still holds the structures each fingerprint is there for (a changed generator would lose them silently)."""
    def plans(fp, planner):
        return PC.decode(_get(_get(_get(_get(_get(gold, 'fingerprints'), fp), 'planners'), planner), 'plans'))
    for planner in PLANNERS[:3]:
        assert plans('ct_large', planner)['num_stages'] == 2
    v21 = _stages(plans('ct_large', 'ExperimentPlanner3D_v21'))
    assert list(v21[1]['patch_size']) == [64, 160, 192] and v21[1]['conv_kernel_sizes'][0] == [1, 3, 3]
    mt = plans('ct_large', 'ExperimentPlanner3D_v21_MultiTalent')
    assert mt['base_num_features'] == 30 and all(s['batch_size'] == 4 for s in _stages(mt))
    assert list(_stages(mt)[1]['current_spacing']) == [1.5, 1.0, 1.0] and list(_stages(mt)[1]['patch_size']) == [128, 192, 192]
    small = plans('ct_small', 'ExperimentPlanner3D_v21')
    s = _stages(small)[0]
    assert small['num_stages'] == 1 and small['transpose_forward'] == [2, 0, 1] and len(s['pool_op_kernel_sizes']) == 4
    assert any(p > m for p, m in zip(s['patch_size'], s['median_patient_size_in_voxels']))
    an = plans('aniso', 'ExperimentPlanner3D_v21')
    s = _stages(an)[0]
    assert len(s['pool_op_kernel_sizes']) == 6 and s['do_dummy_2D_data_aug'] and an['normalization_schemes'][0] == 'nonCT'
    fp = PC.decode(_get(_get(_get(gold, 'fingerprints'), 'aniso'), 'dataset_properties'))
    assert s['current_spacing'][0] < np.median(np.vstack(fp['all_spacings'])[:, 0])         # the anisotropy rule moved the target
    b = _stages(plans('aniso', 'ExperimentPlanner'))[0]
    assert [1, 1, 3] in b['conv_kernel_sizes'] and [1, 2, 1] in b['pool_op_kernel_sizes']
    br = plans('brain4', 'ExperimentPlanner3D_v21')
    assert list(br['normalization_schemes'].values()) == ['nonCT'] * 3 + ['noNorm'] and br['transpose_forward'] == [1, 0, 2]
    assert all(br['use_mask_for_norm'].values())
    la = plans('last_axis', 'ExperimentPlanner3D_v21')
    s = _stages(la)[0]
    assert la['transpose_forward'] == [2, 0, 1] and la['num_classes'] == 13 and s['do_dummy_2D_data_aug']
    assert s['pool_op_kernel_sizes'][:2] == [[1, 2, 2]] * 2 and s['conv_kernel_sizes'][:2] == [[1, 3, 3]] * 2
    res = _stages(plans('ct_small', 'ExperimentPlanner3DFabiansResUNet_v21'))[0]
    assert res['pool_op_kernel_sizes'][0] == [1, 1, 1] and len(res['num_blocks_encoder']) == len(res['pool_op_kernel_sizes'])


def test_pool_and_conv_props_table(gold):
    rows = PC.decode(_get(gold, 'props'))
    assert len(rows) >= 200
    small = ratio_lo = ratio_hi = 0
    for spacing, patch, cap, want_late, want_v21 in rows:
        spacing = [float(i) for i in spacing.split()]
        late = common_utils.get_pool_and_conv_props_poolLateV2(list(patch), 4, cap, np.array(spacing))
        v21 = common_utils.get_pool_and_conv_props(np.array(spacing), list(patch), 4, cap)
        assert PC.pack_topology(late) == want_late, (spacing, patch, cap)
        assert PC.pack_topology(v21) == want_v21, (spacing, patch, cap)
        assert all(isinstance(r[3], np.ndarray) and isinstance(r[4], np.ndarray) for r in (late, v21))
        small += min(patch) < 8
        q = max(spacing) / min(spacing)
        ratio_lo += q < 2
        ratio_hi += q > 2
    assert small > 10 and ratio_lo > 10 and ratio_hi > 10          # patches below 2 * min_feature_map_size, ratios on both sides of 2


def test_vram_table(gold, capsys):
    rows = PC.decode(_get(gold, 'vram'))
    assert len(rows) >= 24
    for r in rows:
        pool = [[int(i) for i in k] for k in r['pools'].split()]
        plain = Generic_UNet.compute_approx_vram_consumption(r['patch'], list(np.sum(np.array(pool) == 2, 0)), r['base'], r['max'],
                                                             r['modalities'], r['classes'], pool, r['deep_supervision'],
                                                             r['conv_per_stage'])
        assert type(plain).__name__ == r['plain_type'] and int(plain) == r['plain'], r
        pk = [[1, 1, 1]] + pool
        res = FabiansUNet.compute_approx_vram_consumption(r['patch'], r['base'], r['max'], r['modalities'], r['classes'], pk,
                                                          FabiansUNet.default_blocks_per_stage_encoder[:len(pk)],
                                                          FabiansUNet.default_blocks_per_stage_decoder[:len(pk) - 1], 2, 2)
        assert float(res).hex() == float(r['residual']).hex(), r
    assert Generic_UNet.use_this_for_batch_size_computation_3D == 520000000 and Generic_UNet.BASE_NUM_FEATURES_3D == 30
    assert Generic_UNet.MAX_NUM_FILTERS_3D == 320 and Generic_UNet.DEFAULT_BATCH_SIZE_3D == 2
    assert Generic_UNet.DEFAULT_PATCH_SIZE_3D == (64, 192, 160) and FabiansUNet.use_this_for_batch_size_computation_3D == 727842816.0


def test_pretrained_flow(gold, tmp_path, capsys):
    """The plans of one dataset as `-overwrite_plans` of another: the file keeps the target's name and `num_classes`, takes the new
    data identifier, and everything else is the source's."""
    rec = _get(gold, 'pretrained')
    fps = _get(gold, 'fingerprints')
    source = PC.fingerprint_of(_get(fps, _get(rec, 'source')))
    target = PC.fingerprint_of(_get(fps, _get(rec, 'target')))
    src, sroots = _plan('ExperimentPlanner3D_v21', source, tmp_path / 's')
    planner, roots = _plan('ExperimentPlanner3D_v21_Pretrained', target, tmp_path / 't', (src.plans_fname, 'GOLD'))
    assert isinstance(planner, ExperimentPlanner3D_v21_Pretrained)
    assert os.path.basename(planner.plans_fname) == _get(rec, 'fname') == 'nnUNetPlans_pretrained_GOLD_plans_3D.pkl'
    v21 = PC.decode(_get(_get(_get(_get(fps, _get(rec, 'target')), 'planners'), 'ExperimentPlanner3D_v21'), 'plans'))
    with open(planner.plans_fname, 'rb') as f:                      # before the preprocessing: this dataset's own plan (-no_pp)
        own = PC.compact_plans(PC.relativize(pickle.load(f), roots), target)
    v21.update(PC.decode(_get(rec, 'own_differs_from_v21')))
    assert list(PC.decode(_get(rec, 'own_differs_from_v21'))) == ['data_identifier'] and PC.encode(own) == PC.encode(v21)
    planner.load_pretrained_plans()
    capsys.readouterr()
    with open(planner.plans_fname, 'rb') as f:
        plans = pickle.load(f)
    want = PC.decode(_get(_get(_get(_get(fps, _get(rec, 'source')), 'planners'), 'ExperimentPlanner3D_v21'), 'plans'))
    want.update(PC.decode(_get(rec, 'differs_from_source')))
    source_roots = {k: v for k, v in sroots.items()}                # the paths in the file are the source's
    assert PC.encode(PC.compact_plans(PC.relativize(plans, source_roots), source)) == PC.encode(want)
    assert PC.encode(planner.transpose_forward) == _get(rec, 'transpose_forward')
    assert planner.preprocessor_name == _get(rec, 'preprocessor_name')
    with open(src.plans_fname, 'rb') as f:
        sp = pickle.load(f)
    assert plans['data_identifier'] == 'nnUNetData_pretrained_GOLD' and plans['num_classes'] == len(target['dataset_properties']['all_classes'])
    assert plans['num_classes'] != sp['num_classes']
    for k in sp:
        if k not in ('data_identifier', 'num_classes'):
            assert PC.encode(plans[k]) == PC.encode(sp[k]), k


def test_load_my_plans_round_trips(gold, tmp_path, capsys):
    fp = PC.fingerprint_of(_get(_get(gold, 'fingerprints'), 'ct_large'))
    planner, _ = _plan('ExperimentPlanner3D_v21', fp, tmp_path)
    again = ExperimentPlanner3D_v21(planner.folder_with_cropped_data, planner.preprocessed_output_folder)
    again.load_my_plans()
    capsys.readouterr()
    assert PC.encode(again.plans) == PC.encode(planner.plans)
    assert PC.encode(again.plans_per_stage) == PC.encode(planner.plans_per_stage)
    assert again.transpose_forward == planner.transpose_forward and again.transpose_backward == planner.transpose_backward
    assert PC.encode(again.dataset_properties) == PC.encode(planner.dataset_properties)


@pytest.mark.parametrize('fingerprint,stages', [('ct_small', 1), ('ct_large', 2)])
def test_get_default_configuration_reads_the_written_plans(gold, fingerprint, stages, tmp_path, monkeypatch, capsys):
    from multitalent_amd.run.default_configuration import get_default_configuration
    fp = PC.fingerprint_of(_get(_get(gold, 'fingerprints'), fingerprint))
    pre = tmp_path / 'pre'
    cropped, out = str(tmp_path / 'cropped'), str(pre / 'Task555_Gold')
    os.makedirs(out)
    PC.write_fingerprint_folder(cropped, fp)
    ExperimentPlanner3D_v21(cropped, out).plan_experiment()
    capsys.readouterr()
    monkeypatch.setenv('nnUNet_preprocessed', str(pre))
    monkeypatch.setenv('RESULTS_FOLDER', str(tmp_path / 'results'))
    plans_file, output_folder, dataset_directory, batch_dice, stage, trainer_class = \
        get_default_configuration('3d_fullres', 'Task555_Gold', 'nnUNetTrainerV2')
    assert plans_file == os.path.join(out, 'nnUNetPlansv2.1_plans_3D.pkl') and dataset_directory == out
    assert stage == stages - 1 and batch_dice == (stages > 1) and trainer_class.__name__ == 'nnUNetTrainerV2'


def test_every_planner_is_found_by_name():
    for name in PLANNERS + ('ExperimentPlanner3D_v21_Pretrained',):
        cls = driver._find_planner(name)
        assert cls.__name__ == name and cls.__module__.startswith('multitalent_amd.experiment_planning')
    with pytest.raises(RuntimeError, match="Could not find the Planner class ExperimentPlanner3D_v99"):
        driver._find_planner('ExperimentPlanner3D_v99')


def test_driver_refusals_come_before_any_file_is_touched(monkeypatch, tmp_path):
    for var in ('nnUNet_raw_data_base', 'nnUNet_preprocessed', 'RESULTS_FOLDER'):
        monkeypatch.delenv(var, raising=False)                      # any access to a folder would raise RuntimeError instead
    with pytest.raises(NotImplementedError, match="-pl2d None"):
        driver.main(['-t', '901'])                                  # the default -pl2d is ExperimentPlanner2D_v21
    with pytest.raises(NotImplementedError, match="-pl2d None"):
        driver.main(['-t', '901', '-pl2d', 'ExperimentPlanner2D_v21', '-pl3d', 'None'])
    with pytest.raises(AssertionError, match="-pl3d ExperimentPlanner3D_v21_Pretrained"):
        driver.main(['-t', '901', '-pl2d', 'None', '-overwrite_plans', str(tmp_path / 'p.pkl'), '-overwrite_plans_identifier', 'X'])
    with pytest.raises(AssertionError, match="You need to specify -overwrite_plans_identifier"):
        driver.main(['-t', '901', '-pl2d', 'None', '-pl3d', 'ExperimentPlanner3D_v21_Pretrained', '-overwrite_plans',
                     str(tmp_path / 'p.pkl')])
    with pytest.raises(RuntimeError, match="nnUNet_raw_data_base is not defined"):
        driver.main(['-t', '901', '-pl2d', 'None'])


def test_task_name_lookup_searches_all_roots(monkeypatch, tmp_path):
    from multitalent_amd import paths
    from multitalent_amd.utilities.task_name_id_conversion import convert_id_to_task_name, convert_task_name_to_id
    base, pre, res = tmp_path / 'base', tmp_path / 'pre', tmp_path / 'res'
    monkeypatch.setenv('nnUNet_raw_data_base', str(base))
    monkeypatch.setenv('nnUNet_preprocessed', str(pre))
    monkeypatch.setenv('RESULTS_FOLDER', str(res))
    assert paths.nnUNet_raw_data() == str(base / 'nnUNet_raw_data') and paths.nnUNet_cropped_data() == str(base / 'nnUNet_cropped_data')
    assert paths.preprocessing_output_dir() == str(pre) and paths.network_training_output_dir() == str(res / 'nnUNet')
    for d in (base / 'nnUNet_raw_data' / 'Task007_Seven', base / 'nnUNet_cropped_data' / 'Task007_Seven', pre / 'Task008_Eight',
              res / 'nnUNet' / '3d_fullres' / 'Task009_Nine', base / 'nnUNet_raw_data' / 'Task010_Ten', pre / 'Task010_Zehn'):
        os.makedirs(d)
    assert convert_id_to_task_name(7) == 'Task007_Seven' and convert_id_to_task_name(8) == 'Task008_Eight'
    assert convert_id_to_task_name(9) == 'Task009_Nine' and convert_task_name_to_id('Task009_Nine') == 9
    with pytest.raises(RuntimeError, match="More than one task name found for task id 10"):
        convert_id_to_task_name(10)
    with pytest.raises(RuntimeError, match="Could not find a task with the ID 11"):
        convert_id_to_task_name(11)
    monkeypatch.delenv('nnUNet_raw_data_base')
    assert paths.nnUNet_raw_data() is None and convert_id_to_task_name(8) == 'Task008_Eight'
    with pytest.raises(RuntimeError, match="nnUNet_raw_data_base"):
        paths.require(paths.nnUNet_cropped_data)
    monkeypatch.setenv('nnUNet_raw_data_base', str(tmp_path / 'not_there'))              # a root that does not exist yet holds no task
    monkeypatch.setenv('RESULTS_FOLDER', str(tmp_path / 'not_there_either'))
    assert convert_id_to_task_name(8) == 'Task008_Eight'
