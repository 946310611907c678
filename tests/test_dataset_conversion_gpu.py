"""The Task100 journey on the device: `mt_label_convert` for each stored type against the numpy restatement and the REAL reference's
results (tests/golden/dataset_conversion.*), its report of unexpected values, the NIfTI wrapper, and the chain of the reference's
readme at toy size: convert_task100 -> verify_dataset_integrity -> nnUNet_plan_and_preprocess -t 100 -> add_regions ->
MultiTalent_trainer_ddp / run_training.main.  Labels are integers: every comparison of volumes is exact."""
import os
import pickle
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_conversion_cases as CC  # noqa: E402
import planning_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
ABDOMEN = (tuple(range(1, 14)), tuple(range(10, 23)))          # Task017's map: 13 labels, all of them fit int8
GUARD, POISON = 67, 0xAB                                       # an odd margin: the output base is misaligned as well


@pytest.fixture(scope='module')
def reference(dev):
    """One label volume for every size and type, and what it becomes: computed once, never changed."""
    from multitalent_amd import ops
    n = max(ops.label_convert_round(d) for d in CC.DTYPES) + 4099
    rs = np.random.RandomState(17)
    labels = rs.randint(0, 14, size=n).astype(np.uint8)
    labels[rs.rand(n) < 0.6] = 0                               # mostly background, as label maps are
    labels[:14] = np.arange(14)
    want, unexpected, _ = CC.np_convert(labels, *ABDOMEN)
    assert unexpected == 0
    labels.setflags(write=False)
    want.setflags(write=False)
    return labels, want


def _convert_view(ops, values, offset, table):
    """values (numpy, any of the eight types) placed `offset` elements into an allocation -> (result, count, smallest) with the
    output inside poisoned guard margins, which are checked."""
    V = values.size
    host = np.zeros(V + 4, dtype=values.dtype)
    host[offset:offset + V] = values
    buf = torch.from_numpy(host).cuda()
    seg = buf[offset:offset + V]
    assert seg.data_ptr() == buf.data_ptr() + offset * values.dtype.itemsize
    out = torch.full((V + 2 * GUARD + 4,), POISON, dtype=torch.uint8, device=buf.device)
    view = out[GUARD + offset:GUARD + offset + V]
    got, count, smallest = ops.label_convert(seg, table, out=view)
    assert got.data_ptr() == view.data_ptr()
    host_out = out.cpu().numpy()
    assert (host_out[:GUARD + offset] == POISON).all() and (host_out[GUARD + offset + V:] == POISON).all()
    return host_out[GUARD + offset:GUARD + offset + V], count, smallest


@pytest.mark.parametrize('dtype', CC.DTYPES)
def test_label_convert_every_type_size_and_alignment(dev, reference, dtype):
    from multitalent_amd import ops
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import label_table
    labels, want = reference
    table = label_table(*ABDOMEN)
    round_ = ops.label_convert_round(dtype)
    per_thread = 8 if dtype == 'float64' else 16
    assert round_ == torch.cuda.get_device_properties(dev).multi_processor_count * 8 * 256 * per_thread
    for V in (1, 385, 4099, round_ + 4099):                    # the last: a full round of the grid-stride loop and a part of the next
        values = labels[:V].astype(dtype)
        for offset in range(4):
            got, count, smallest = _convert_view(ops, values, offset, table)
            assert (count, smallest) == (0, None), (dtype, V, offset)
            assert np.array_equal(got, want[:V]), (dtype, V, offset)
    assert np.array_equal(_convert_view(ops, labels[1:2].astype(dtype), 1, table)[0], [10])       # V = 1 that is not background
    # the reference's own results for the same values in this type (5 x 7 x 11 voxels)
    meta, z = CC.golden()
    for c in meta['cases']:
        vol = z[c['name'] + '/in']
        if c['raises'] is not None or not np.array_equal(vol, vol.astype(dtype).astype(np.float64), equal_nan=True):
            continue                                           # values this type cannot hold
        got, count, _ = ops.label_convert(torch.from_numpy(vol.astype(dtype)).to(dev), label_table(c['labels_in'], c['labels_out']))
        assert tuple(got.shape) == vol.shape and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), z[c['name'] + '/out']), (dtype, c['name'])
        assert count == 0 or not c['sanity_check']


def test_label_convert_rejects_bad_arguments(dev):
    from multitalent_amd import ops
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import label_table
    table = label_table((1,), (2,))
    seg = torch.zeros(8, dtype=torch.int16, device=dev)
    bad = table.copy()
    bad[5] = 300
    with pytest.raises(RuntimeError, match='no uint8 value'):
        ops.label_convert(seg, bad)
    with pytest.raises(ValueError):
        ops.label_convert(seg.long(), table)
    with pytest.raises(ValueError):
        ops.label_convert(seg, table[:100])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.label_convert(seg.cpu(), table)


def _planted(dtype):
    """A volume of several blocks with legal labels 0..2, the reference-legal oddities and offenders planted all over it."""
    rs = np.random.RandomState(5)
    n = 300007
    v = rs.randint(0, 3, size=n).astype(dtype)
    where = rs.permutation(n)
    if np.dtype(dtype).kind == 'f':
        legal = [np.nan, -1.0, 1e-21, -np.inf, -0.0]
        offenders = [7.0, 2.5, np.inf, 1e30, 1023.0, 3.0]
    else:
        legal = [-1, -70000, 0]
        offenders = [7, 70000, 1023, 3]
    v[where[:500]] = np.resize(np.array(legal, dtype=dtype), 500)
    v[where[500:1500]] = np.resize(np.array(offenders, dtype=dtype), 1000)
    only_legal = v.copy()
    only_legal[where[500:1500]] = 1
    return v, only_legal, min(offenders)


@pytest.mark.parametrize('dtype', ['float32', 'int32', 'float64'])
def test_unexpected_values_are_counted_and_the_smallest_is_reported(dev, dtype):
    from multitalent_amd import ops
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import copy_and_convert_segmentation, label_table
    v, only_legal, smallest_planted = _planted(dtype)
    labels_in, labels_out = (1, 2), (4, 5)
    want, n, smallest = CC.np_convert(v, labels_in, labels_out)
    assert n == 1000 and smallest == float(np.dtype(dtype).type(smallest_planted))
    seg = torch.from_numpy(v).to(dev)
    first = ops.label_convert(seg, label_table(labels_in, labels_out))
    second = ops.label_convert(seg, label_table(labels_in, labels_out))
    assert (first[1], first[2]) == (n, smallest)
    assert np.float64(first[2]).tobytes() == np.float64(second[2]).tobytes() and first[1] == second[1]      # bit-identical reports
    assert torch.equal(first[0], second[0]) and np.array_equal(first[0].cpu().numpy(), want)
    with pytest.raises(RuntimeError) as e:
        copy_and_convert_segmentation(v, labels_in, labels_out, True, '/data/labelsTr/case_7.nii.gz')
    assert '/data/labelsTr/case_7.nii.gz' in str(e.value) and repr(smallest) in str(e.value) and '[1, 2]' in str(e.value)
    got = copy_and_convert_segmentation(v, labels_in, labels_out, sanity_check=False)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
    # NaN, negatives and 1e-21 alone raise nothing
    clean = copy_and_convert_segmentation(only_legal, labels_in, labels_out, True, 'legal')
    assert np.array_equal(clean, CC.np_convert(only_legal, labels_in, labels_out)[0])
    on_device = copy_and_convert_segmentation(torch.from_numpy(only_legal).to(dev), labels_in, labels_out)
    assert torch.is_tensor(on_device) and on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), clean)


def test_the_references_offenders_and_wide_integers(dev):
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import copy_and_convert_segmentation
    meta, z = CC.golden()
    by_name = {c['name']: c for c in meta['cases']}
    for name in ('offenders', 'unlisted_sanity'):
        c = by_name[name]
        with pytest.raises(RuntimeError) as e:
            copy_and_convert_segmentation(z[name + '/in'], c['labels_in'], c['labels_out'], True, name)
        assert repr(float(c['raises'])) in str(e.value)                               # the value the reference met first
    c = by_name['offenders_no_sanity']
    assert np.array_equal(copy_and_convert_segmentation(z[c['name'] + '/in'], c['labels_in'], c['labels_out'], False), z[c['name'] + '/out'])
    wide = np.array([[0, 1, 2, -5, 2 ** 40]], dtype=np.int64)                         # cast to float64 on the host, as get_fdata does
    with pytest.raises(RuntimeError):
        copy_and_convert_segmentation(wide, (1, 2), (4, 5))
    assert np.array_equal(copy_and_convert_segmentation(wide, (1, 2), (4, 5), False), [[0, 4, 5, 0, 0]])
    assert np.array_equal(copy_and_convert_segmentation(wide.astype(np.uint64)[:, :3], (1, 2), (4, 5)), [[0, 4, 5]])


def test_copy_and_convert_segmentation_nifti_keeps_the_geometry(dev, tmp_path):
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import copy_and_convert_segmentation_nifti
    from multitalent_amd.preprocessing.sanity_checks import verify_same_geometry
    from multitalent_amd.utilities.nifti_io import read_image, write_image
    a, b = np.deg2rad(20.0), np.deg2rad(-35.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    geo = dict(spacing=(0.78125, 0.6875, 2.5), origin=(-112.5, 37.25, -401.0), direction=tuple((Rz @ Rx).ravel()))
    rs = np.random.RandomState(3)
    seg = rs.randint(0, 3, size=(9, 13, 17)).astype(np.int16)
    src, img, dst = str(tmp_path / 'liver_1.nii.gz'), str(tmp_path / 'liver_1_0000.nii.gz'), str(tmp_path / '003_liver_1.nii.gz')
    write_image(seg, src, **geo)
    write_image(rs.randn(9, 13, 17).astype(np.float32), img, **geo)
    copied = str(tmp_path / '003_liver_1_0000.nii.gz')
    shutil.copy(img, copied)
    copy_and_convert_segmentation_nifti(src, dst, (1, 2), (7, 9))
    got = read_image(dst)
    assert np.asarray(got.array).dtype == np.uint8
    assert np.array_equal(np.asarray(got.array), CC.np_convert(seg, (1, 2), (7, 9))[0])
    assert verify_same_geometry(read_image(copied), got)                              # spacing, origin, direction, size
    assert not np.allclose(got.GetDirection(), np.eye(3).ravel(), atol=0.1) and np.allclose(got.GetSpacing(), geo['spacing'])
    bad = seg.copy()
    bad[4, 4, 4] = 5
    write_image(bad, src, **geo)
    target = str(tmp_path / 'never.nii.gz')
    with pytest.raises(RuntimeError, match='liver_1.nii.gz'):
        copy_and_convert_segmentation_nifti(src, target, (1, 2), (7, 9))
    assert not os.path.exists(target)


# ---- the chain at toy size ---------------------------------------------------------------------------------------------------------
def _case(i, shape, spacing, margin, seg_dtype):
    return dict(id=i, shape=shape, spacing=spacing, margin=margin, seg_dtype=seg_dtype)


SOURCES = [       # one label, two labels, two labels with a Val split
    dict(name='Task009_Spleen', modality='CT', labels=2, seed=9, cases=[
        _case('spleen_2', (40, 44, 18), (0.75, 0.75, 3.0), ((3, 2), (4, 4), (1, 2)), 'uint8'),
        _case('spleen_10', (42, 40, 20), (0.8125, 0.8125, 3.0), ((2, 2), (0, 5), (2, 2)), 'float32')]),
    dict(name='Task007_Pancreas', modality='CT', labels=3, seed=7, cases=[
        _case('pancreas_001', (38, 46, 18), (0.75, 0.75, 2.5), ((0, 3), (5, 3), (0, 3)), 'int16'),
        _case('pancreas_004', (40, 42, 16), (0.6875, 0.6875, 3.0), ((4, 0), (2, 2), (2, 0)), 'float64')]),
    dict(name='Task003_Liver', modality='CT', labels=3, seed=3, cases=[
        _case('liver_0', (44, 44, 20), (0.75, 0.75, 3.5), ((2, 4), (3, 3), (3, 1)), 'int16'),
        _case('liver_3', (40, 44, 18), (0.75, 0.75, 3.0), ((1, 2), (2, 4), (1, 1)), 'int32')]),
]
LIVER_VAL = dict(name='Task003_Liver', modality='CT', labels=3, seed=33, cases=[
    _case('liver_9', (40, 40, 16), (0.75, 0.75, 3.0), ((2, 2), (2, 2), (1, 1)), 'uint16')])
TASK = 'Task100_MultiTalent'


@pytest.fixture(scope='module')
def chain(dev, tmp_path_factory):
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import convert_task100
    from multitalent_amd.dataset_conversion.Task100_MultiTalent_addregions import add_regions
    from multitalent_amd.preprocessing.sanity_checks import verify_dataset_integrity
    root = tmp_path_factory.mktemp('task100_chain')
    e = PC.ToyEnvironment(root)
    for task in SOURCES:
        PC.write_toy_task(e.raw, task)
    val = PC.write_toy_task(str(root / 'val_source'), LIVER_VAL)
    shutil.move(os.path.join(val, 'imagesTr'), os.path.join(e.raw, 'Task003_Liver', 'imagesVal'))
    shutil.move(os.path.join(val, 'labelsTr'), os.path.join(e.raw, 'Task003_Liver', 'labelsVal'))
    e.tasks = [t['name'] for t in SOURCES]
    e.plan = convert_task100(tasks=e.tasks, num_threads=2)
    e.target = os.path.join(e.raw, TASK)
    verify_dataset_integrity(e.target)
    e.plan_and_preprocess(dict(name=TASK), '-pl3d', 'ExperimentPlanner3D_v21_MultiTalent')
    e.updated = add_regions()
    yield e
    e.close()


def test_chain_conversion_writes_the_merged_task(chain):
    from multitalent_amd.dataset_conversion import Task100_MultiTalent as T
    from multitalent_amd.utilities.nifti_io import read_image
    assert len(chain.plan['copy']) == 7 and len(chain.plan['convert']) == 7
    with open(os.path.join(chain.target, 'cases_have_regions_labels.pkl'), 'rb') as f:
        l_tr, l_val, l_ts, r_tr, r_val, r_ts = pickle.load(f)
    assert sorted(l_tr) == ['003_liver_0.nii.gz', '003_liver_3.nii.gz', '007_pancreas_001.nii.gz', '007_pancreas_004.nii.gz',
                            '009_spleen_10.nii.gz', '009_spleen_2.nii.gz']
    assert l_val == {'003_liver_9.nii.gz': (1, 2)} and r_val == {'003_liver_9.nii.gz': ('03_liver', '03_cancer')} and l_ts == r_ts == {}
    assert l_tr['007_pancreas_004.nii.gz'] == (4, 5) and r_tr['009_spleen_2.nii.gz'] == ('09_spleen',)
    for src, dst, labels_in, labels_out in chain.plan['convert']:
        a, b = read_image(src), read_image(dst)
        assert np.asarray(b.array).dtype == np.uint8
        assert np.array_equal(np.asarray(b.array), CC.np_convert(np.asarray(a.array), labels_in, labels_out)[0]), dst
        assert set(np.unique(np.asarray(b.array))) == {0} | set(labels_out)
    for src, dst in chain.plan['copy']:
        assert open(src, 'rb').read() == open(dst, 'rb').read()
    assert os.path.isfile(os.path.join(chain.target, 'imagesVal', '003_liver_9_0000.nii.gz'))
    assert sorted(os.listdir(os.path.join(chain.target, 'imagesTs'))) == []
    # a second run finds everything in place
    again = T.plan_conversion(chain.raw, chain.tasks)
    assert again['copy'] == [] and again['convert'] == [] and again['dictionaries'] == chain.plan['dictionaries']


def test_chain_every_preprocessed_case_carries_its_regions(chain):
    from multitalent_amd.dataset_conversion import Task100_MultiTalent as T
    out = os.path.join(chain.preprocessed, TASK)
    stages = sorted(d for d in os.listdir(out) if d.startswith('MultiTalent_data_stage'))
    assert len(stages) >= 1 and os.path.isfile(os.path.join(out, 'MultiTalent_bs4_plans_3D.pkl'))
    assert chain.updated == 6 * (1 + len(stages))
    by_id = {t[4:7]: t for t in chain.tasks}
    for folder in [os.path.join(out, s) for s in stages] + [os.path.join(chain.cropped, TASK)]:
        cases = PC.load_cases(folder)
        assert len(cases) == 6
        for key, (data, props) in cases.items():
            source = by_id[key[:3]]
            assert tuple(props['valid_regions']) == T.MultiTalent_valid_regions[source]
            assert tuple(props['valid_labels']) == tuple(T.MultiTalent_task_label_maps[source][1])
            assert set(np.unique(data[-1])) <= {-1.0, 0.0} | {float(i) for i in T.MultiTalent_task_label_maps[source][1]}
            assert set(np.unique(data[-1])) & {float(i) for i in T.MultiTalent_task_label_maps[source][1]}


@pytest.fixture(scope='module')
def pg():
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29583')
    os.environ.setdefault('RANK', '0'); os.environ.setdefault('WORLD_SIZE', '1')
    created = not dist.is_initialized()
    if created:
        dist.init_process_group('nccl', init_method='env://')
    yield
    if created:
        dist.destroy_process_group()


def test_chain_multitalent_trainer_runs_an_iteration(chain, pg):
    from multitalent_amd.run.default_configuration import get_default_configuration
    plans_file, output_folder, dataset_directory, batch_dice, stage, trainer_class = \
        get_default_configuration('3d_fullres', TASK, 'MultiTalent_trainer_ddp', 'MultiTalent_bs4')
    tr = trainer_class(plans_file, 'all', 0, output_folder=output_folder, dataset_directory=dataset_directory, batch_dice=batch_dice,
                       stage=stage, unpack_data=True, deterministic=False, fp16=False)
    os.makedirs(tr.output_folder, exist_ok=True)
    tr.initialize(True)
    assert tr.num_classes == 47 and tr.folder_with_preprocessed_data.endswith('MultiTalent_data_stage%d' % stage)
    tr.setup_data_generators()
    tr.network.train()
    np.random.seed(100)
    loss = tr.run_iteration(tr.tr_gen, True)
    assert np.isfinite(np.asarray([float(i) for i in (loss if isinstance(loss, tuple) else (loss,))])).all()


def test_chain_nnunet_train_entry(chain, monkeypatch):
    """`nnUNet_train 3d_fullres nnUNetTrainerV2 100 all -p MultiTalent_bs4`, cut to two iterations.  Task100's dataset.json declares
    47 labels, so this is a 48-class softmax network: the loss runs on the wave-per-voxel softmax Dice + CE kernels
    (tests/test_softmax_loss_wide_gpu.py)."""
    from multitalent_amd.run import run_training
    from multitalent_amd.training.model_restore import find_trainer_class
    cls = find_trainer_class('nnUNetTrainerV2')
    orig = cls.run_training

    def short(self):
        self.max_num_epochs, self.num_batches_per_epoch, self.num_val_batches_per_epoch, self.save_every = 1, 2, 1, 1
        return orig(self)

    monkeypatch.setattr(cls, 'run_training', short)
    np.random.seed(0)
    run_training.main(['3d_fullres', 'nnUNetTrainerV2', '100', 'all', '-p', 'MultiTalent_bs4', '--fp32', '--disable_postprocessing_on_folds'])
    out = os.path.join(chain.results, 'nnUNet', '3d_fullres', TASK, 'nnUNetTrainerV2__MultiTalent_bs4', 'all')
    files = set(os.listdir(out))
    assert {'model_final_checkpoint.model', 'model_final_checkpoint.model.pkl', 'validation_raw'} <= files
    ck = torch.load(os.path.join(out, 'model_final_checkpoint.model'), map_location='cpu', weights_only=False)
    assert ck['epoch'] == 1
    predicted = [f for f in os.listdir(os.path.join(out, 'validation_raw')) if f.endswith('.nii.gz')]
    assert sorted(predicted) == sorted(k[:-7] + '.nii.gz' for k in chain.plan['dictionaries'][0])


def test_nnunet_train_entry_on_a_source_task(chain, monkeypatch):
    """The same entry on a task the softmax loss can hold: Task007_Pancreas of the same tree (3 classes), planned with v2.1:
    `nnUNet_train 3d_fullres nnUNetTrainerV2 7 all`, then `-val --val_folder again` from the final checkpoint."""
    from multitalent_amd.run import run_training
    from multitalent_amd.training.model_restore import find_trainer_class
    chain.plan_and_preprocess(SOURCES[1], '-pl3d', 'ExperimentPlanner3D_v21')
    cls = find_trainer_class('nnUNetTrainerV2')
    orig = cls.run_training

    def short(self):
        self.max_num_epochs, self.num_batches_per_epoch, self.num_val_batches_per_epoch, self.save_every = 1, 2, 1, 1
        return orig(self)

    monkeypatch.setattr(cls, 'run_training', short)
    np.random.seed(0)
    run_training.main(['3d_fullres', 'nnUNetTrainerV2', '7', 'all', '--fp32', '--disable_postprocessing_on_folds'])
    out = os.path.join(chain.results, 'nnUNet', '3d_fullres', 'Task007_Pancreas', 'nnUNetTrainerV2__nnUNetPlansv2.1', 'all')
    assert {'model_final_checkpoint.model', 'model_final_checkpoint.model.pkl', 'validation_raw'} <= set(os.listdir(out))
    ck = torch.load(os.path.join(out, 'model_final_checkpoint.model'), map_location='cpu', weights_only=False)
    assert ck['epoch'] == 1
    want = sorted(c['id'] + '.nii.gz' for c in SOURCES[1]['cases'])
    assert sorted(f for f in os.listdir(os.path.join(out, 'validation_raw')) if f.endswith('.nii.gz')) == want
    run_training.main(['3d_fullres', 'nnUNetTrainerV2', 'Task007_Pancreas', 'all', '--fp32', '-val', '--val_folder', 'again',
                       '--disable_postprocessing_on_folds'])
    assert sorted(f for f in os.listdir(os.path.join(out, 'again')) if f.endswith('.nii.gz')) == want
