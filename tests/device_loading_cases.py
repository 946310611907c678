"""What tests/test_device_loading_cpu.py and tests/test_device_loading_gpu.py share: the golden loader folder (rebuilt as
tests/test_dataset_loading.py does), numpy's crop + pad of one patch, and small synthetic two-modality cases."""
import os
import pickle

import numpy as np

from test_dataset_loading import CONFIGS, G, _write  # noqa: F401

SEEDS, BATCHES = range(4), 2
SYNTH_SHAPES = ((7, 19, 13), (15, 22, 27))
SYNTH_PATCH = (11, 23, 21)                       # PW % 4 != 0; larger than the first case in every axis, than the second in one


def np_patch(case, bb_lb, patch_size, pad_mode):
    """case [C+1, x, y, z], lower corner bb_lb -> (data [C, *patch], seg [1, *patch]) as generate_train_batch builds them."""
    shape = case.shape[1:]
    bb_ub = [bb_lb[d] + patch_size[d] for d in range(3)]
    vlb = [max(0, bb_lb[d]) for d in range(3)]
    vub = [min(shape[d], bb_ub[d]) for d in range(3)]
    crop = np.copy(case[:, vlb[0]:vub[0], vlb[1]:vub[1], vlb[2]:vub[2]])
    pads = ((0, 0),) + tuple((-min(0, bb_lb[d]), max(bb_ub[d] - shape[d], 0)) for d in range(3))
    return np.pad(crop[:-1], pads, pad_mode), np.pad(crop[-1:], pads, 'constant', constant_values=-1)


def golden_loader_args(ds, p, ci):
    """(positional, keyword) constructor arguments of golden configuration ci."""
    ps, fps, B, ov, pm, pad_sides, use_p = CONFIGS[ci]
    return (ds, ps, fps, B, False), dict(oversample_foreground_percent=ov, pad_mode=pm, pad_sides=pad_sides, memmap_mode='r',
                                         sampling_probabilities=p if use_p else None)


def write_synthetic(folder, n_per_shape=2, seed=7):
    """C = 2 cases of SYNTH_SHAPES, labels -1..3, as .npz + .npy + .pkl."""
    rng = np.random.RandomState(seed)
    for s, shape in enumerate(SYNTH_SHAPES):
        for k in range(n_per_shape):
            data = rng.standard_normal((2,) + shape).astype(np.float32)
            seg = rng.randint(-1, 4, shape).astype(np.float32)
            arr = np.concatenate([data, seg[None]], 0)
            name = 'SYN%d_%02d' % (s, k)
            np.savez_compressed(os.path.join(folder, name + '.npz'), data=arr)
            np.save(os.path.join(folder, name + '.npy'), arr)
            with open(os.path.join(folder, name + '.pkl'), 'wb') as f:
                pickle.dump({'class_locations': {c: np.argwhere(seg == c) for c in (1, 2, 3)}}, f)
