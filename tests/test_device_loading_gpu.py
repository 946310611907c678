"""The device loader on the device (csrc/loader.hip, training/dataloading/device_loading.py).  Everything is a copy, so every comparison
is `np.array_equal`: `DeviceDataLoader3D` against the golden batches of tests/golden/loader.npz (cases smaller than the patch in some
axes and larger in others, odd widths, one case without foreground; constant and edge padding, oversized patches, pad_sides) under
three cache budgets and both storages; against the host `DataLoader3D` (which those goldens pin to the reference) on two-modality cases
with a patch of PW % 4 != 0, more than one launch and guard margins around the outputs; `mt_seg_narrow`; the augmenter over either
loader; the trainer's choice of loader."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_loading_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden(tmp_path_factory):
    """The golden folder in both storages, written once: {unpack: (dataset, sqrt probabilities)} and the golden file."""
    from multitalent_amd.training.dataloading import dataset_loading as dl
    z = np.load(DC.G)
    out = {}
    for unpack in (True, False):
        d = tmp_path_factory.mktemp('npy' if unpack else 'npz')
        DC._write(str(d), z, unpack)
        ds = dl.load_dataset(str(d))
        out[unpack] = (ds, dl.sqrt_sampling_probabilities(ds.keys())[0])
    return out, z


def _check_goldens(ds, p, z, cache_for):
    from multitalent_amd.training.dataloading.device_loading import DeviceDataLoader3D
    for ci in range(len(DC.CONFIGS)):
        for seed in DC.SEEDS:
            args, kw = DC.golden_loader_args(ds, p, ci)
            np.random.seed(seed)
            loader = DeviceDataLoader3D(*args, cache=cache_for(ci, seed), **kw)
            for it in range(DC.BATCHES):
                b = next(loader)
                k = 'cfg%d/seed%d/it%d/' % (ci, seed, it)
                assert [str(x) for x in b['keys']] == [str(x) for x in z[k + 'keys']], k
                assert b['data'].is_cuda and b['data'].dtype == torch.float32 and b['seg'].dtype == torch.float32
                assert np.array_equal(b['data'].cpu().numpy(), z[k + 'data']), k
                assert np.array_equal(b['seg'].cpu().numpy(), z[k + 'seg']), k
                assert len(b['properties']) == args[3] and 'valid_regions' in b['properties'][0]


@pytest.mark.parametrize('unpack', [True, False])
@pytest.mark.parametrize('budget', ['all', 'none'])
def test_device_loader_reproduces_golden_batches(dev, golden, unpack, budget):
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache
    (ds, p), z = golden[0][unpack], golden[1]
    cache = DeviceCaseCache(dev, 1 << 30 if budget == 'all' else 0)       # one cache for all configurations: cases stay resident
    _check_goldens(ds, p, z, lambda ci, seed: cache)
    total = sum(DeviceCaseCache.case_bytes(z[k].shape) for k in z.files if k.startswith('case/'))
    if budget == 'all':
        assert len(cache) == 6 and cache.used_bytes == total
    else:
        assert len(cache) == 0 and cache.used_bytes == 0


@pytest.mark.parametrize('unpack', [True, False])
def test_budget_for_exactly_the_first_two_cases(dev, golden, unpack):
    """C = 1: a case takes 6 V bytes.  A budget of 6 (V_a + V_b) for the first two distinct cases a run draws holds exactly those."""
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache
    (ds, p), z = golden[0][unpack], golden[1]
    caches = []

    def cache_for(ci, seed):
        first = []
        for it in range(DC.BATCHES):
            for key in z['cfg%d/seed%d/it%d/keys' % (ci, seed, it)]:
                if str(key) not in first:
                    first.append(str(key))
        a, b = (int(np.prod(z['case/' + k].shape[1:])) for k in first[:2])
        caches.append((DeviceCaseCache(dev, 6 * (a + b)), [ds[k]['data_file'] for k in first[:2]]))
        return caches[-1][0]

    _check_goldens(ds, p, z, cache_for)
    for cache, files in caches:
        assert len(cache) == 2 and sorted(cache.resident_files()) == sorted(files) and cache.used_bytes == cache.budget_bytes


GUARD, SENTINEL = 4099, -12345.0


def _guarded(dev, shape):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return flat, flat[GUARD:GUARD + n].view(shape)


@pytest.fixture(scope='module')
def synthetic(tmp_path_factory):
    from multitalent_amd.training.dataloading import dataset_loading as dl
    d = tmp_path_factory.mktemp('synthetic')
    DC.write_synthetic(str(d))
    return dl.load_dataset(str(d))


@pytest.mark.parametrize('budget', ['all', 'none'])
@pytest.mark.parametrize('pad_mode', ['constant', 'edge'])
@pytest.mark.parametrize('B', [3, 17])
def test_two_modalities_odd_patch_many_samples_equal_the_host_loader(dev, synthetic, B, pad_mode, budget):
    from multitalent_amd.training.dataloading import dataset_loading as dl
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache, DeviceDataLoader3D
    ps = DC.SYNTH_PATCH
    kw = dict(oversample_foreground_percent=0.5, pad_mode=pad_mode, memmap_mode='r')
    np.random.seed(11)
    host = dl.DataLoader3D(synthetic, ps, ps, B, False, **kw)
    want = [next(host) for _ in range(2)]
    np.random.seed(11)
    loader = DeviceDataLoader3D(synthetic, ps, ps, B, False, cache=DeviceCaseCache(dev, 1 << 30 if budget == 'all' else 0), **kw)
    drawn = set()
    for w in want:
        drawn.update(str(k) for k in w['keys'])
        dflat, dview = _guarded(dev, (B, 2) + ps)
        sflat, sview = _guarded(dev, (B, 1) + ps)
        b = loader.generate_train_batch(data_out=dview, seg_out=sview)
        assert b['data'].data_ptr() == dview.data_ptr() and b['seg'].data_ptr() == sview.data_ptr()
        assert [str(k) for k in b['keys']] == [str(k) for k in w['keys']]
        assert np.array_equal(b['data'].cpu().numpy(), w['data'])
        assert np.array_equal(b['seg'].cpu().numpy(), w['seg'])
        for flat in (dflat, sflat):
            assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all())
    assert len(loader.cache) == (len(drawn) if budget == 'all' else 0)


def test_seg_narrow_round_trip_and_flag(dev):
    from multitalent_amd import ops
    labels = torch.arange(-1, 105, dtype=torch.float32, device=dev).repeat(13)[:1375].contiguous()       # V % 4 != 0: quads and a tail
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.seg_narrow(labels, flag)
    assert out.dtype == torch.int16 and int(flag.item()) == 0 and torch.equal(out.float(), labels)
    for bad in (0.5, 40000.0, float('nan')):
        for pos in (3, 1374):
            x = labels.clone()
            x[pos] = bad
            flag.zero_()
            ops.seg_narrow(x, flag)
            assert int(flag.item()) == 1, (bad, pos)


@pytest.mark.parametrize('bad', [0.5, 40000.0])
@pytest.mark.parametrize('budget', ['all', 'none'])
def test_loader_refuses_labels_that_int16_cannot_hold(dev, tmp_path, bad, budget):
    import pickle
    from multitalent_amd.training.dataloading import dataset_loading as dl
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache, DeviceDataLoader3D
    arr = np.zeros((2, 8, 8, 8), dtype=np.float32)
    arr[1, 4, 4, 4] = bad
    np.savez_compressed(str(tmp_path / 'BAD_00.npz'), data=arr)
    with open(str(tmp_path / 'BAD_00.pkl'), 'wb') as f:
        pickle.dump({'class_locations': {1: np.zeros((0, 3), dtype=np.int64)}}, f)
    np.random.seed(0)
    loader = DeviceDataLoader3D(dl.load_dataset(str(tmp_path)), (8, 8, 8), (8, 8, 8), 1, pad_mode='constant',
                                cache=DeviceCaseCache(dev, 1 << 20 if budget == 'all' else 0))
    with pytest.raises(RuntimeError, match='BAD_00'):
        next(loader)


def test_augmenter_over_device_and_host_loader_agree(dev, golden):
    from multitalent_amd.training.data_augmentation.color import MoreDADeviceAugmenter, default_3d_augmentation_params
    from multitalent_amd.training.data_augmentation.spatial import get_patch_size
    from multitalent_amd.training.dataloading import dataset_loading as dl
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache, DeviceDataLoader3D
    (ds, p), _ = golden[0][True], golden[1]
    params = default_3d_augmentation_params()
    ps = (12, 24, 24)
    bps = tuple(int(i) for i in get_patch_size(ps, params['rotation_x'], params['rotation_y'], params['rotation_z'], (0.85, 1.25)))
    kw = dict(oversample_foreground_percent=0.33, pad_mode='constant', memmap_mode='r', sampling_probabilities=p)
    got = []
    for cls, extra in ((dl.DataLoader3D, {}), (DeviceDataLoader3D, {'cache': DeviceCaseCache(dev, 1 << 30)})):
        np.random.seed(5)
        torch.manual_seed(5)
        aug = MoreDADeviceAugmenter(cls(ds, bps, ps, 2, False, **kw, **extra), ps, params, dev)
        got.append([next(aug) for _ in range(3)])
    for h, d in zip(*got):
        assert [str(k) for k in h['keys']] == [str(k) for k in d['keys']]
        assert tuple(d['data'].shape) == (2, 1) + ps
        assert np.array_equal(h['data'].cpu().numpy(), d['data'].cpu().numpy(), equal_nan=True)
        assert np.array_equal(h['target'].cpu().numpy(), d['target'].cpu().numpy())


def test_trainer_builds_device_loaders(dev, tmp_path):
    from multitalent_amd import plans as P
    from multitalent_amd.training.dataloading.dataset_loading import DataLoader3D
    from multitalent_amd.training.dataloading.device_loading import DeviceDataLoader3D
    from multitalent_amd.training.model_restore import find_trainer_class
    z = np.load(DC.G)
    sp = {'batch_size': 2, 'patch_size': np.array([12, 24, 24]), 'pool_op_kernel_sizes': [[2, 2, 2], [2, 2, 2]],
          'conv_kernel_sizes': [[3, 3, 3]] * 3, 'do_dummy_2D_data_aug': False}
    plans = P.make_plans(sp, base_num_features=8, num_classes=47, stage=1)
    folder = tmp_path / (plans['data_identifier'] + '_stage1')
    folder.mkdir()
    DC._write(str(folder), z, unpack=False)
    tr = find_trainer_class('nnUNetTrainerV2')(plans, 0, output_folder=None, dataset_directory=str(tmp_path), stage=1)
    tr.load_plans_file(); tr.process_plans(tr.plans)
    assert tr.device_dataloading is True
    tr.setup_augmentation_params()
    dl_tr, dl_val = tr.get_basic_generators()
    assert type(dl_tr) is DeviceDataLoader3D and type(dl_val) is DeviceDataLoader3D and dl_tr.cache is dl_val.cache
    assert tuple(dl_tr.patch_size) == tuple(int(i) for i in tr.basic_generator_patch_size) and tuple(dl_val.patch_size) == (12, 24, 24)
    assert dl_tr.sampling_probabilities is None and dl_tr.batch_size == 2
    total = torch.cuda.get_device_properties(dev).total_memory
    assert dl_tr.cache.budget_bytes == int(tr.device_case_cache_fraction * total)
    np.random.seed(0)
    b = next(dl_val)
    assert b['data'].is_cuda and tuple(b['data'].shape) == (2, 1, 12, 24, 24) and tuple(b['seg'].shape) == (2, 1, 12, 24, 24)
    tr.device_dataloading = False
    dl_tr, dl_val = tr.get_basic_generators()
    assert type(dl_tr) is DataLoader3D and type(dl_val) is DataLoader3D
    # the MultiTalent trainers inherit the attribute and keep their sqrt sampling
    import torch.distributed as dist
    from multitalent_amd.training.dataloading.dataset_loading import sqrt_sampling_probabilities
    for k, v in (('MASTER_ADDR', '127.0.0.1'), ('MASTER_PORT', '29633'), ('RANK', '0'), ('WORLD_SIZE', '1')):
        os.environ.setdefault(k, v)
    own_group = not dist.is_initialized()
    mt = find_trainer_class('MultiTalent_trainer_ddp')(plans, 'all', 0, output_folder=None, dataset_directory=str(tmp_path), stage=1)
    try:
        mt.load_plans_file(); mt.process_plans(mt.plans)
        mt.setup_augmentation_params()
        dl_tr, dl_val = mt.get_basic_generators()
        assert type(dl_tr) is DeviceDataLoader3D and type(dl_val) is DeviceDataLoader3D and dl_tr.cache is dl_val.cache
        assert tuple(dl_tr.patch_size) == tuple(int(i) for i in mt.basic_generator_patch_size) and tuple(dl_val.patch_size) == (12, 24, 24)
        assert np.array_equal(dl_tr.sampling_probabilities, sqrt_sampling_probabilities(list(mt.dataset_tr.keys()))[0])
    finally:
        if own_group and dist.is_initialized():
            dist.destroy_process_group()
