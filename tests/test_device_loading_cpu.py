"""Host half of the device loader (training/dataloading/device_loading.py), no GPU: `plan_batch` makes the host loader's draws (keys,
boxes and the numpy random state after every batch equal DataLoader3D's; a numpy crop + pad from the plan equals the golden batches
of tests/golden/loader.npz), and the index / pad function the gather kernel compiles (csrc/patch_index.h) equals numpy's crop + pad
when a stand-alone host program, built with the address and undefined-behaviour sanitizers, gathers with it into exact-size buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_loading_cases as DC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize('unpack', [True, False])
def test_plan_batch_makes_the_host_loaders_draws(tmp_path, unpack):
    from multitalent_amd.training.dataloading import dataset_loading as dl
    from multitalent_amd.training.dataloading.device_loading import DeviceDataLoader3D
    z = np.load(DC.G)
    DC._write(str(tmp_path), z, unpack)
    ds = dl.load_dataset(str(tmp_path))
    p, _ = dl.sqrt_sampling_probabilities(ds.keys())
    for ci in range(len(DC.CONFIGS)):
        ps, pad_mode = DC.CONFIGS[ci][0], DC.CONFIGS[ci][4]
        for seed in DC.SEEDS:
            args, kw = DC.golden_loader_args(ds, p, ci)
            np.random.seed(seed)
            host = dl.DataLoader3D(*args, **kw)
            states = []
            for it in range(DC.BATCHES):
                next(host)
                states.append(np.random.get_state())
            np.random.seed(seed)
            loader = DeviceDataLoader3D(*args, **kw)
            assert tuple(loader.patch_size) == tuple(ps) and loader.batch_size == args[3] and loader.pad_mode == pad_mode
            for it in range(DC.BATCHES):
                plan = loader.plan_batch()
                k = 'cfg%d/seed%d/it%d/' % (ci, seed, it)
                assert _same_state(np.random.get_state(), states[it]), k
                assert [str(x) for x in plan['keys']] == [str(x) for x in z[k + 'keys']], k
                assert len(plan['properties']) == args[3] and 'valid_regions' in plan['properties'][0]
                data, seg = [], []
                for key, lb, shape in zip(plan['keys'], plan['bb_lb'], plan['shapes']):
                    case = z['case/' + str(key)]
                    assert tuple(shape) == case.shape[1:]
                    a, b = DC.np_patch(case, lb, ps, pad_mode)
                    data.append(a); seg.append(b)
                assert np.array_equal(np.stack(data), z[k + 'data']), k
                assert np.array_equal(np.stack(seg), z[k + 'seg']), k


def test_device_loader_rejects_what_it_does_not_do(tmp_path):
    from multitalent_amd.training.dataloading import dataset_loading as dl
    from multitalent_amd.training.dataloading.device_loading import DeviceDataLoader3D
    DC._write(str(tmp_path), np.load(DC.G), True)
    ds = dl.load_dataset(str(tmp_path))
    with pytest.raises(NotImplementedError):
        DeviceDataLoader3D(ds, (12, 24, 24), (12, 24, 24), 2, True)
    with pytest.raises(NotImplementedError):
        DeviceDataLoader3D(ds, (12, 24, 24), (12, 24, 24), 2, pad_mode='reflect')


# lower corners: all before the case, all past its end, mixed, and wholly inside where the case is larger than the patch
HOST_CASES = [(DC.SYNTH_SHAPES[0], (-2, -2, -4)), (DC.SYNTH_SHAPES[0], (-4, -1, 0)), (DC.SYNTH_SHAPES[0], (0, -4, -8)), (DC.SYNTH_SHAPES[0], (3, 10, 7)),
              (DC.SYNTH_SHAPES[1], (0, -1, 0)), (DC.SYNTH_SHAPES[1], (4, -1, 6)), (DC.SYNTH_SHAPES[1], (2, 0, 3)), (DC.SYNTH_SHAPES[1], (-5, 11, -9)),
              (DC.SYNTH_SHAPES[1], (9, 14, 20))]


def test_index_function_under_sanitizers_equals_numpy_pad(tmp_path):
    exe = str(tmp_path / 'patch_gather_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', os.path.join(ROOT, 'multitalent_amd', 'csrc'), os.path.join(ROOT, 'tests', 'patch_gather_host.cpp'), '-o', exe])
    C, ps = 2, DC.SYNTH_PATCH
    pv = ps[0] * ps[1] * ps[2]
    for shape, lb in HOST_CASES:
        v = shape[0] * shape[1] * shape[2]
        case = np.stack([np.arange(v, dtype=np.float32).reshape(shape) + 100000 * c for c in range(C)]
                        + [(np.arange(v) % 7 - 1).astype(np.float32).reshape(shape)])
        for mode, name in ((0, 'constant'), (1, 'edge')):
            out = str(tmp_path / 'out.bin')
            r = subprocess.run([exe, str(C)] + [str(i) for i in shape + lb + ps] + [str(mode), out], capture_output=True, text=True)
            assert r.returncode == 0, (shape, lb, name, r.stderr[-2000:])
            got = np.fromfile(out, dtype=np.float32)
            assert got.size == (C + 1) * pv
            data, seg = DC.np_patch(case, lb, ps, name)
            assert np.array_equal(got[:C * pv].reshape((C,) + ps), data), (shape, lb, name)
            assert np.array_equal(got[C * pv:].reshape((1,) + ps), seg), (shape, lb, name)
