"""The host half of the Task100 journey, no GPU: the label table against the REAL reference function
(tests/golden/dataset_conversion.*) and a numpy restatement; the voxel classification of csrc/label_class.h as a stand-alone host
program under the address and undefined-behaviour sanitizers; `sanity_checks`; the plan of a conversion run on a fabricated raw
tree; `generate_dataset_json` against the reference's; `add_regions`; and the call sequence of `run_training.main`."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_conversion_cases as CC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_label_table_equals_the_reference_mapping():
    from multitalent_amd.dataset_conversion import Task100_MultiTalent as T
    meta, z = CC.golden()
    names = [c['name'] for c in meta['cases']]
    assert set(T.MultiTalent_task_label_maps) <= set(names) and {'example', 'entry0', 'repeated'} <= set(names)
    for c in meta['cases']:
        table = T.label_table(c['labels_in'], c['labels_out'])
        assert table.dtype == np.uint16 and table.shape == (CC.SLOTS,)
        assert np.array_equal(table, CC.np_table(c['labels_in'], c['labels_out'])), c['name']
        # the reference applied to every label 0..1022 once: an unlisted label becomes 0 there
        assert np.array_equal(np.where(table == CC.UNLISTED, 0, table).astype(np.uint8), z[c['name'] + '/table']), c['name']
        assert table[0] == CC.UNLISTED
    t = T.label_table((1, 2, (3, 4), 3), (4, 5, 6, 7))
    assert [int(t[i]) for i in (1, 2, 3, 4)] == [4, 5, 7, 6] and (np.delete(t, [1, 2, 3, 4]) == CC.UNLISTED).all()
    assert int(T.label_table((0, 1), (9, 8))[0]) == CC.UNLISTED                      # an entry 0 never applies
    assert int(T.label_table((1, 1, (1, 2)), (3, 4, 5))[1]) == 5                     # the last pair wins
    for t_name, (li, lo) in T.MultiTalent_task_label_maps.items():
        table = T.label_table(li, lo)
        assert [int(table[i]) for i in li] == list(lo) and int((table != CC.UNLISTED).sum()) == len(li), t_name


def test_label_table_rejects_what_does_not_fit():
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import copy_and_convert_segmentation, label_table
    for bad_in, bad_out in (((1,), (256,)), ((1, 2), (3, -1)), ((1023,), (1,)), (((1, 5000),), (1,)), ((-1,), (1,)), ((1, 2), (1,)),
                            ((1.0,), (1,)), ((1,), (1.5,))):
        with pytest.raises(ValueError):
            label_table(bad_in, bad_out)
    assert int(label_table((1022,), (255,))[1022]) == 255
    with pytest.raises(ValueError):                                                  # before any device is asked for
        copy_and_convert_segmentation(np.zeros((2, 2, 2), dtype=np.uint8), (1,), (300,))


def test_numpy_restatement_equals_the_reference():
    """The restatement the device tests compare with is itself checked against the real function's results."""
    meta, z = CC.golden()
    for c in meta['cases']:
        out, n, smallest = CC.np_convert(z[c['name'] + '/in'], c['labels_in'], c['labels_out'])
        if c['raises'] is not None:
            assert c['sanity_check'] and n > 0 and smallest == float(c['raises']), c['name']
        else:
            assert np.array_equal(out, z[c['name'] + '/out']), c['name']
            assert n == 0 or not c['sanity_check'], c['name']
    by_name = {c['name']: c for c in meta['cases']}
    assert by_name['offenders']['raises'] == '0.5' and by_name['legal_specials']['raises'] is None


# ---- the classification header -----------------------------------------------------------------------------------------------------
FLOATS = [0.0, -1.0, 1e-21, 1e-20, np.nan, np.inf, -np.inf, 2.5, 2.0, 1022.0, 1023.0, 1e30, -0.0, 0.5, 1.0, 1021.5, 1022.5, 5e-324, 1e-19]


def test_classification_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'label_class_host')
    subprocess.check_call(['/opt/rocm/bin/hipcc' if os.path.isfile('/opt/rocm/bin/hipcc') else 'hipcc', '--offload-arch=gfx950', '-O1', '-g',
                           '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                           '-I', os.path.join(ROOT, 'multitalent_amd', 'csrc'), os.path.join(ROOT, 'tests', 'label_class_host.cpp'), '-o', exe])
    for name in CC.DTYPES:
        dt = np.dtype(name)
        if dt.kind == 'f':
            with np.errstate(over='ignore', under='ignore'):
                vals = np.array(FLOATS, dtype=dt)
            vals = np.concatenate([vals, np.nextafter(np.array([1e-20, 1022.0], dtype=dt), dt.type(np.inf)),
                                   np.array([np.finfo(dt).max, np.finfo(dt).tiny], dtype=dt)])
        else:
            info = np.iinfo(dt)
            vals = np.array([v for v in (info.min, info.min + 1, -1, 0, 1, 2, 127, 128, 255, 256, 1022, 1023, 1024, 70000, info.max - 1, info.max)
                             if info.min <= v <= info.max], dtype=dt)
        src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
        vals.tofile(src)
        r = subprocess.run([exe, name, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        raw = open(dst, 'rb').read()
        assert len(raw) == 12 * vals.size
        slot = np.frombuffer(raw[:4 * vals.size], dtype=np.int32)
        key = np.frombuffer(raw[4 * vals.size:], dtype=np.uint64)
        assert np.array_equal(slot, CC.np_slot(vals)), (name, vals, slot)
        assert np.array_equal(key, vals.astype(np.float64).view(np.uint64)), name
        # the key orders the values that can be unexpected (everything above 1e-20) as the numbers do
        up = vals.astype(np.float64)[slot != -1]
        assert np.array_equal(np.argsort(up, kind='stable'), np.argsort(key[slot != -1], kind='stable')), name
    f32 = CC.np_slot(np.array(FLOATS, dtype=np.float32))
    assert list(f32[:12]) == [-1, -1, -1, -1, -1, -2, -1, -2, 2, 1022, -2, -2]


# ---- the driver's host functions -------------------------------------------------------------------------------------------------
def test_sanity_checks_pass_on_the_packaged_tables():
    from multitalent_amd.dataset_conversion import Task100_MultiTalent as T
    T.sanity_checks()
    assert len(T.MultiTalent_task_label_maps) == 13


def _touch(folder, names):
    os.makedirs(folder)
    for n in names:
        open(os.path.join(folder, n), 'wb').close()


@pytest.fixture
def raw_tree(tmp_path):
    raw = str(tmp_path / 'nnUNet_raw_data')
    _touch(os.path.join(raw, 'Task009_Spleen', 'imagesTr'), ['spleen_2_0000.nii.gz', 'spleen_10_0000.nii.gz', 'readme.txt'])
    _touch(os.path.join(raw, 'Task009_Spleen', 'labelsTr'), ['spleen_2.nii.gz', 'spleen_10.nii.gz'])
    _touch(os.path.join(raw, 'Task003_Liver', 'imagesTr'), ['liver_0_0000.nii.gz'])
    _touch(os.path.join(raw, 'Task003_Liver', 'labelsTr'), ['liver_0.nii.gz'])
    _touch(os.path.join(raw, 'Task003_Liver', 'imagesVal'), ['liver_5_0000.nii.gz'])
    _touch(os.path.join(raw, 'Task003_Liver', 'labelsVal'), ['liver_5.nii.gz'])
    _touch(os.path.join(raw, 'Task017_AbdominalOrganSegmentation', 'imagesTr'), ['img0001_0000.nii.gz'])
    _touch(os.path.join(raw, 'Task017_AbdominalOrganSegmentation', 'labelsTr'), ['img0001.nii.gz'])
    _touch(os.path.join(raw, 'Task017_AbdominalOrganSegmentation', 'imagesTs'), ['img0061_0000.nii.gz'])
    _touch(os.path.join(raw, 'Task017_AbdominalOrganSegmentation', 'labelsTs'), ['img0061.nii.gz'])
    return raw


TASKS = ['Task009_Spleen', 'Task003_Liver', 'Task017_AbdominalOrganSegmentation']


def test_plan_conversion_on_a_fabricated_tree(raw_tree):
    from multitalent_amd.dataset_conversion import Task100_MultiTalent as T
    j = os.path.join
    base = j(raw_tree, 'Task100_MultiTalent')
    plan = T.plan_conversion(raw_tree, TASKS)
    assert plan['target_base'] == base
    assert plan['folders'] == {k: j(base, k) for k in ('imagesTr', 'labelsTr', 'imagesVal', 'labelsVal', 'imagesTs', 'labelsTs')}
    assert plan['copy'] == [
        (j(raw_tree, 'Task009_Spleen', 'imagesTr', 'spleen_10_0000.nii.gz'), j(base, 'imagesTr', '009_spleen_10_0000.nii.gz')),
        (j(raw_tree, 'Task009_Spleen', 'imagesTr', 'spleen_2_0000.nii.gz'), j(base, 'imagesTr', '009_spleen_2_0000.nii.gz')),
        (j(raw_tree, 'Task003_Liver', 'imagesTr', 'liver_0_0000.nii.gz'), j(base, 'imagesTr', '003_liver_0_0000.nii.gz')),
        (j(raw_tree, 'Task003_Liver', 'imagesVal', 'liver_5_0000.nii.gz'), j(base, 'imagesVal', '003_liver_5_0000.nii.gz')),
        (j(raw_tree, 'Task017_AbdominalOrganSegmentation', 'imagesTr', 'img0001_0000.nii.gz'), j(base, 'imagesTr', '017_img0001_0000.nii.gz')),
        (j(raw_tree, 'Task017_AbdominalOrganSegmentation', 'imagesTs', 'img0061_0000.nii.gz'), j(base, 'imagesTs', '017_img0061_0000.nii.gz'))]
    abdomen = (tuple(range(1, 14)), tuple(range(10, 23)))
    assert plan['convert'] == [
        (j(raw_tree, 'Task009_Spleen', 'labelsTr', 'spleen_10.nii.gz'), j(base, 'labelsTr', '009_spleen_10.nii.gz'), (1,), (8,)),
        (j(raw_tree, 'Task009_Spleen', 'labelsTr', 'spleen_2.nii.gz'), j(base, 'labelsTr', '009_spleen_2.nii.gz'), (1,), (8,)),
        (j(raw_tree, 'Task003_Liver', 'labelsTr', 'liver_0.nii.gz'), j(base, 'labelsTr', '003_liver_0.nii.gz'), (1, 2), (1, 2)),
        (j(raw_tree, 'Task003_Liver', 'labelsVal', 'liver_5.nii.gz'), j(base, 'labelsVal', '003_liver_5.nii.gz'), (1, 2), (1, 2)),
        (j(raw_tree, 'Task017_AbdominalOrganSegmentation', 'labelsTr', 'img0001.nii.gz'), j(base, 'labelsTr', '017_img0001.nii.gz')) + abdomen,
        (j(raw_tree, 'Task017_AbdominalOrganSegmentation', 'labelsTs', 'img0061.nii.gz'), j(base, 'labelsTs', '017_img0061.nii.gz')) + abdomen]
    l_tr, l_val, l_ts, r_tr, r_val, r_ts = plan['dictionaries']
    assert l_tr == {'009_spleen_10.nii.gz': (8,), '009_spleen_2.nii.gz': (8,), '003_liver_0.nii.gz': (1, 2), '017_img0001.nii.gz': abdomen[1]}
    assert l_val == {'003_liver_5.nii.gz': (1, 2)} and l_ts == {'017_img0061.nii.gz': abdomen[1]}
    assert r_tr == {'009_spleen_10.nii.gz': ('09_spleen',), '009_spleen_2.nii.gz': ('09_spleen',), '003_liver_0.nii.gz': ('03_liver', '03_cancer'),
                    '017_img0001.nii.gz': T.MultiTalent_valid_regions['Task017_AbdominalOrganSegmentation']}
    assert r_val == {'003_liver_5.nii.gz': ('03_liver', '03_cancer')}
    assert r_ts == {'017_img0061.nii.gz': T.MultiTalent_valid_regions['Task017_AbdominalOrganSegmentation']}
    assert len(r_tr['017_img0001.nii.gz']) == 13
    # a target that exists is not done again, but stays in the dictionaries; `overwrite` takes it back in
    _touch(j(base, 'labelsTr'), ['009_spleen_2.nii.gz'])
    _touch(j(base, 'labelsVal'), ['003_liver_5.nii.gz'])
    _touch(j(base, 'imagesTr'), ['003_liver_0_0000.nii.gz'])
    again = T.plan_conversion(raw_tree, TASKS)
    assert [c for c in plan['convert'] if c not in again['convert']] == [plan['convert'][1], plan['convert'][3]]
    assert [c for c in plan['copy'] if c not in again['copy']] == [plan['copy'][2]]
    assert again['dictionaries'] == plan['dictionaries']
    assert T.plan_conversion(raw_tree, TASKS, overwrite=True)['convert'] == plan['convert']
    with pytest.raises(RuntimeError, match='missing task: Task006_Lung'):
        T.plan_conversion(raw_tree)                                                  # tasks=None: all 13


def test_convert_task100_has_no_cpu_fallback(raw_tree, monkeypatch):
    import torch
    from multitalent_amd.dataset_conversion import Task100_MultiTalent as T
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)                   # the behaviour without a device, wherever this runs
    monkeypatch.setenv('nnUNet_raw_data_base', os.path.dirname(raw_tree))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        T.convert_task100(tasks=TASKS)
    assert not os.path.exists(os.path.join(raw_tree, 'Task100_MultiTalent'))
    with pytest.raises(RuntimeError, match='missing task'):
        T.convert_task100()


def test_generate_dataset_json_equals_the_reference(tmp_path):
    from multitalent_amd.dataset_conversion import Task100_MultiTalent as T
    from multitalent_amd.dataset_conversion.utils import generate_dataset_json, get_identifiers_from_splitted_files
    meta, _ = CC.golden()
    _touch(str(tmp_path / 'imagesTr'), meta['imagesTr'] + ['notes.txt'])
    _touch(str(tmp_path / 'imagesTs'), meta['imagesTs'] + ['notes.txt'])
    ids = get_identifiers_from_splitted_files(str(tmp_path / 'imagesTr'))
    assert list(ids) == sorted(i[:-12] for i in meta['imagesTr'])
    out = str(tmp_path / 'dataset.json')
    generate_dataset_json(out, str(tmp_path / 'imagesTr'), str(tmp_path / 'imagesTs'), ("CT",), {int(k): v for k, v in T.MultiTalent_labels.items()},
                          "Task100_MultiTalent")
    with open(out) as f:
        assert json.load(f) == meta['dataset_json']
    generate_dataset_json(out, str(tmp_path / 'imagesTr'), None, ("CT", "MR"), {0: 'background', 1: 'x'}, "Other", license="mine",
                          dataset_description="d", dataset_reference="r", dataset_release='1.1')
    with open(out) as f:
        got = json.load(f)
    assert got == meta['dataset_json_no_test'] and got['test'] == [] and got['numTest'] == 0


# ---- add_regions -----------------------------------------------------------------------------------------------------------------
def _dump(obj, fname):
    with open(fname, 'wb') as f:
        pickle.dump(obj, f)


def _load(fname):
    with open(fname, 'rb') as f:
        return pickle.load(f)


def test_add_regions_on_fabricated_folders(tmp_path, monkeypatch):
    from multitalent_amd.dataset_conversion.Task100_MultiTalent_addregions import add_regions
    base, pre = tmp_path / 'base', tmp_path / 'pre'
    task = 'Task100_MultiTalent'
    raw = base / 'nnUNet_raw_data' / task
    cropped = base / 'nnUNet_cropped_data' / task
    stages = [pre / task / 'MultiTalent_data_stage0', pre / task / 'MultiTalent_data_stage1']
    for d in [raw, cropped] + stages + [pre / task / 'gt_segmentations']:
        os.makedirs(str(d))
    cases = ['009_spleen_2', '003_liver_0']
    labels_tr = {'009_spleen_2.nii.gz': (8,), '003_liver_0.nii.gz': (1, 2)}
    regions_tr = {'009_spleen_2.nii.gz': ('09_spleen',), '003_liver_0.nii.gz': ('03_liver', '03_cancer')}
    _dump((labels_tr, {'x.nii.gz': (1,)}, {}, regions_tr, {'x.nii.gz': ('03_liver',)}, {}), str(raw / 'cases_have_regions_labels.pkl'))
    dataset_level = {}
    for d in [cropped] + stages:
        for c in cases:
            _dump({'original_spacing': np.array([1.0, 2.0, 3.0]), 'case': c}, str(d / (c + '.pkl')))
            open(str(d / (c + '.npz')), 'wb').close()
        for n in ('dataset_properties.pkl', 'intensityproperties.pkl'):
            _dump({'all_classes': [1, 2, 8]}, str(d / n))
            dataset_level[str(d / n)] = open(str(d / n), 'rb').read()
    _dump({'plans': 1}, str(pre / task / 'MultiTalent_plans_3D.pkl'))                  # a file, not a sub-folder: not touched
    monkeypatch.setenv('nnUNet_raw_data_base', str(base))
    monkeypatch.setenv('nnUNet_preprocessed', str(pre))
    assert add_regions() == 6
    for d in [cropped] + stages:
        for c in cases:
            props = _load(str(d / (c + '.pkl')))
            assert props['valid_labels'] == labels_tr[c + '.nii.gz'] and props['valid_regions'] == regions_tr[c + '.nii.gz']
            assert props['case'] == c and np.array_equal(props['original_spacing'], [1.0, 2.0, 3.0])
    for fname, content in dataset_level.items():
        assert open(fname, 'rb').read() == content
    assert _load(str(pre / task / 'MultiTalent_plans_3D.pkl')) == {'plans': 1}
    _dump({'case': 'stranger'}, str(stages[1] / '006_lung_1.pkl'))
    with pytest.raises(KeyError):
        add_regions()


# ---- run_training ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def stub_run(tmp_path, monkeypatch):
    """run_training.main with a trainer class found by name that records what is done to it."""
    from multitalent_amd.run import run_training
    from multitalent_amd.training.network_training.nnUNetTrainer import nnUNetTrainer, nnUNetTrainerV2_DDP
    calls = []

    class Net(object):
        def eval(self):
            calls.append(('network.eval',))

    class StubTrainer(nnUNetTrainer):
        def __init__(self, *args, **kwargs):
            calls.append(('init', args, kwargs))
            self.network = Net()

        def initialize(self, training=True):
            calls.append(('initialize', training))

    for name in ('load_latest_checkpoint', 'run_training', 'load_best_checkpoint', 'load_final_checkpoint', 'validate', 'find_lr'):
        setattr(StubTrainer, name, (lambda n: lambda self, *a, **k: calls.append((n, a, k)))(name))

    class StubDDP(nnUNetTrainerV2_DDP):
        def __init__(self, *args, **kwargs):
            calls.append(('ddp init',))

    def configuration(network, task, network_trainer, plans_identifier):
        calls.append(('configuration', network, task, network_trainer, plans_identifier))
        cls = {'StubTrainer': StubTrainer, 'StubDDP': StubDDP}[network_trainer]
        return 'plans.pkl', 'out_folder', 'data_dir', True, 1, cls

    monkeypatch.setattr(run_training, 'get_default_configuration', configuration)
    monkeypatch.setattr(run_training, 'load_pretrained_weights', lambda net, fname: calls.append(('load_pretrained_weights', type(net).__name__, fname)))
    monkeypatch.setattr(run_training, 'convert_id_to_task_name', lambda i: 'Task%03d_Found' % i)
    return run_training, calls


EXPECTED_VALIDATE = dict(save_softmax=False, validation_folder_name='validation_raw', run_postprocessing_on_folds=True, overwrite=True)


def test_run_training_plain_run(stub_run):
    run_training, calls = stub_run
    run_training.main(['3d_fullres', 'StubTrainer', '902', '3', '-p', 'MY_PLANS'])
    assert calls[0] == ('configuration', '3d_fullres', 'Task902_Found', 'StubTrainer', 'MY_PLANS')
    assert calls[1] == ('init', ('plans.pkl', 3), dict(output_folder='out_folder', dataset_directory='data_dir', batch_dice=True, stage=1,
                                                        unpack_data=True, deterministic=False, fp16=True))
    assert 'local_rank' not in calls[1][2] and len(calls[1][1]) == 2
    assert calls[2:] == [('initialize', True), ('run_training', (), {}), ('network.eval',), ('validate', (), EXPECTED_VALIDATE)]


def test_run_training_fp32_fold_all_and_ignored_flags(stub_run):
    run_training, calls = stub_run
    run_training.main(['3d_fullres', 'StubTrainer', 'Task100_MultiTalent', 'all', '--fp32', '--use_compressed_data', '--deterministic',
                       '--find_lr', '--disable_next_stage_pred', '--disable_postprocessing_on_folds', '--val_disable_overwrite',
                       '--val_folder', 'v', '--disable_saving'])
    assert calls[0][2] == 'Task100_MultiTalent'
    assert calls[1][1] == ('plans.pkl', 'all') and calls[1][2]['fp16'] is False
    assert calls[1][2]['unpack_data'] is False and calls[1][2]['deterministic'] is True
    assert [c[0] for c in calls[2:]] == ['initialize', 'run_training', 'network.eval', 'validate']           # no find_lr call
    assert calls[-1][2] == dict(save_softmax=False, validation_folder_name='v', run_postprocessing_on_folds=False, overwrite=False)


def test_run_training_continue_and_pretrained_weights(stub_run):
    run_training, calls = stub_run
    run_training.main(['3d_fullres', 'StubTrainer', 'Task902_Target', '0', '-c', '-pretrained_weights', 'ignored.model'])
    assert [c[0] for c in calls[2:]] == ['initialize', 'load_latest_checkpoint', 'run_training', 'network.eval', 'validate']
    del calls[:]
    run_training.main(['3d_fullres', 'StubTrainer', 'Task902_Target', '0', '-pretrained_weights', 'source/model_final_checkpoint.model'])
    assert calls[2:5] == [('initialize', True), ('load_pretrained_weights', 'Net', 'source/model_final_checkpoint.model'), ('run_training', (), {})]
    assert [c[0] for c in calls[5:]] == ['network.eval', 'validate']


def test_run_training_validation_only(stub_run):
    run_training, calls = stub_run
    run_training.main(['3d_fullres', 'StubTrainer', 'Task902_Target', '0', '-val', '--valbest', '--npz', '-pretrained_weights', 'unused.model'])
    assert calls[2:] == [('initialize', False), ('load_best_checkpoint', (), {'train': False}), ('network.eval',),
                         ('validate', (), dict(EXPECTED_VALIDATE, save_softmax=True))]
    del calls[:]
    run_training.main(['3d_fullres', 'StubTrainer', 'Task902_Target', '0', '-val'])
    assert calls[2:4] == [('initialize', False), ('load_final_checkpoint', (), {'train': False})]


def test_run_training_refuses_a_ddp_trainer(stub_run):
    run_training, calls = stub_run
    with pytest.raises(RuntimeError, match='run_training_DDP'):
        run_training.main(['3d_fullres', 'StubDDP', 'Task100_MultiTalent', 'all'])
    assert ('ddp init',) not in calls
