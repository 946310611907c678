"""Shared by the planning tests and by tools/oracle_gen/make_golden_planning.py (not a test module): the codec of
tests/golden/planning.json, the folders a planner reads, and the two toy tasks of the device tests.

The codec keeps what the plans are compared on: dict order and keys, list / tuple / ndarray (with its dtype), int, bool, None, str,
and every float tagged and written by `repr`, which round-trips bit for bit.  numpy scalars are stored as the Python value they equal."""
import json
import os
import pickle
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'planning.json')


def encode(o):
    if isinstance(o, (bool, np.bool_)):
        return bool(o)
    if isinstance(o, (int, np.integer)):
        return int(o)
    if isinstance(o, (float, np.floating)):
        return {'f': float(o)}
    if o is None or isinstance(o, str):
        return o
    if isinstance(o, dict):
        return {'dict': [[encode(k), encode(v)] for k, v in o.items()]}
    if isinstance(o, tuple):
        return {'tuple': [encode(i) for i in o]}
    if isinstance(o, list):
        return [encode(i) for i in o]
    if isinstance(o, np.ndarray):
        return {'nd': o.dtype.name, 'v': encode(o.tolist())}
    raise TypeError("planning codec: %r" % type(o))


def decode(o):
    if isinstance(o, list):
        return [decode(i) for i in o]
    if isinstance(o, dict):
        if 'f' in o:
            return float(o['f'])
        if 'dict' in o:
            return OrderedDict((decode(k), decode(v)) for k, v in o['dict'])
        if 'tuple' in o:
            return tuple(decode(i) for i in o['tuple'])
        if 'nd' in o:
            return np.array(decode(o['v']), dtype=o['nd'])
    return o


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def relativize(o, roots):
    """roots: {absolute folder: tag}.  Every string of `o` that starts with a folder has it replaced by its tag."""
    if isinstance(o, str):
        for r, tag in roots.items():
            if o.startswith(r):
                return tag + o[len(r):]
        return o
    if isinstance(o, dict):
        return type(o)((k, relativize(v, roots)) for k, v in o.items())
    if isinstance(o, (list, tuple)):
        return type(o)(relativize(i, roots) for i in o)
    return o


def fingerprint_of(rec):
    """The decoded {'cases', 'dataset_properties'} of a golden fingerprint record."""
    return decode({'dict': [kv for kv in rec['dict'] if kv[0] != 'planners']})


def compact_plans(plans, fp):
    """Plans with relative paths -> a copy in which the four entries that only repeat the fingerprint (`dataset_properties`,
    `original_spacings`, `original_sizes`, `list_of_npz_files`) are replaced by '<fingerprint>' WHERE they equal it; the golden
    file holds this form, and the tests bring their plans into it with the same fingerprint before they compare."""
    dp = fp['dataset_properties']
    same = {'dataset_properties': dp, 'original_spacings': dp['all_spacings'], 'original_sizes': dp['all_sizes'],
            'list_of_npz_files': ['<cropped>/%s.npz' % c for c in fp['cases']]}
    return type(plans)((k, '<fingerprint>' if k in same and encode(v) == encode(same[k]) else v) for k, v in plans.items())


def pack_kernels(kernels):
    """[[1, 2, 2], [2, 2, 2]] -> '122 222'."""
    return ' '.join(''.join(str(int(i)) for i in k) for k in kernels)


def pack_topology(result):
    """The five results of `get_pool_and_conv_props*` in a short form -> 'pools per axis|pool kernels|conv kernels|patch|divisors'."""
    num_pool, pool, conv, patch, divisible = result
    ints = lambda v: ' '.join(str(int(i)) for i in v)
    return '|'.join((ints(num_pool), pack_kernels(pool), pack_kernels(conv), ints(patch), ints(divisible)))


def write_fingerprint_folder(folder, fp):
    """fp: {'cases': [names], 'dataset_properties': {...}} (decoded).  Writes what a planner reads of a cropped folder: an empty
    `<case>.npz` and a small `<case>.pkl` per case, `dataset_properties.pkl`, and a `gt_segmentations` folder."""
    os.makedirs(os.path.join(folder, 'gt_segmentations'), exist_ok=True)
    dp = fp['dataset_properties']
    for i, name in enumerate(fp['cases']):
        open(os.path.join(folder, name + '.npz'), 'wb').close()
        with open(os.path.join(folder, name + '.pkl'), 'wb') as f:
            pickle.dump(OrderedDict(size_after_cropping=dp['all_sizes'][i], original_spacing=dp['all_spacings'][i]), f)
    with open(os.path.join(folder, 'dataset_properties.pkl'), 'wb') as f:
        pickle.dump(dict(dp), f)


def case_mask(folder, cases):
    """The `use_nonzero_mask_for_norm` a planner wrote into every `<case>.pkl` (the same for all cases)."""
    masks = []
    for name in cases:
        with open(os.path.join(folder, name + '.pkl'), 'rb') as f:
            masks.append(pickle.load(f)['use_nonzero_mask_for_norm'])
    assert all(encode(m) == encode(masks[0]) for m in masks)
    return masks[0]


# ---- the toy tasks of the device tests ------------------------------------------------------------------------------------------
# Shapes and spacings in ARRAY order (the coarse axis last, so transpose_forward is not the identity); every spacing is a binary
# fraction, which the float32 header of a NIfTI file holds exactly.  margin: all-zero voxels (lo, hi) per axis around the body.
TASK901 = dict(name='Task901_Tiny', modality='CT', labels=3, seed=901, cases=[
    dict(id='tiny_000', shape=(40, 44, 18), spacing=(0.75, 0.75, 3.0), margin=((3, 2), (4, 4), (1, 2)), seg_dtype='float32'),
    dict(id='tiny_001', shape=(42, 40, 20), spacing=(0.8125, 0.8125, 3.0), margin=((2, 2), (0, 5), (2, 2)), seg_dtype='uint8'),
    dict(id='tiny_002', shape=(38, 46, 18), spacing=(0.75, 0.75, 2.5), margin=((0, 3), (5, 3), (0, 3)), seg_dtype='int16'),
    dict(id='tiny_003', shape=(40, 42, 16), spacing=(0.6875, 0.6875, 3.0), margin=((4, 0), (2, 2), (2, 0)), seg_dtype='int16'),
    dict(id='tiny_004', shape=(44, 44, 20), spacing=(0.75, 0.75, 3.5), margin=((2, 4), (3, 3), (3, 1)), seg_dtype='int16'),
])
TASK902 = dict(name='Task902_Target', modality='CT', labels=4, seed=902, cases=[
    dict(id='target_000', shape=(30, 32, 14), spacing=(1.0, 1.0, 2.5), margin=((2, 2), (2, 3), (1, 1)), seg_dtype='int16'),
    dict(id='target_001', shape=(32, 30, 16), spacing=(1.0, 1.0, 2.5), margin=((1, 3), (2, 2), (2, 1)), seg_dtype='uint8'),
    dict(id='target_002', shape=(28, 34, 14), spacing=(1.125, 1.125, 2.0), margin=((2, 1), (3, 2), (0, 2)), seg_dtype='int16'),
    dict(id='target_003', shape=(30, 30, 16), spacing=(0.875, 0.875, 2.5), margin=((3, 2), (1, 1), (1, 1)), seg_dtype='int16'),
])


def body_shape(case):
    return tuple(int(s - lo - hi) for s, (lo, hi) in zip(case['shape'], case['margin']))


def toy_fingerprint(task):
    """The `dataset_properties` the cropper and the analyzer give for a toy task, without the intensity properties (which come from
    the device and have their own tests): the crop box of a case is its body, because every body voxel is non-zero."""
    dp = dict()
    dp['all_sizes'] = [body_shape(c) for c in task['cases']]
    dp['all_spacings'] = [np.array(c['spacing'], dtype=np.float64) for c in task['cases']]
    dp['all_classes'] = list(range(1, task['labels']))
    dp['modalities'] = {0: task['modality']}
    dp['intensityproperties'] = None
    dp['size_reductions'] = OrderedDict((c['id'], np.prod(body_shape(c)) / np.prod(np.array(c['shape']))) for c in task['cases'])
    return {'cases': [c['id'] for c in task['cases']], 'dataset_properties': dp}


def write_toy_task(raw_data_folder, task):
    """Writes <raw_data_folder>/<task name> with imagesTr, labelsTr and dataset.json (an empty test list) -> the task folder."""
    from multitalent_amd.utilities.nifti_io import write_image
    folder = os.path.join(raw_data_folder, task['name'])
    os.makedirs(os.path.join(folder, 'imagesTr'))
    os.makedirs(os.path.join(folder, 'labelsTr'))
    rs = np.random.RandomState(task['seed'])
    for c in task['cases']:
        body = tuple(slice(lo, s - hi) for s, (lo, hi) in zip(c['shape'], c['margin']))
        bs = body_shape(c)
        img = np.zeros(c['shape'], dtype=np.float32)
        hu = np.round(rs.randn(*bs) * 120 + 60)
        hu[hu == 0] = 1                                               # no zero inside the body: the crop box is the body
        img[body] = hu
        seg = np.zeros(bs, dtype=np.int16)
        for label in range(1, task['labels']):                        # one block per label; a later block may cover an earlier one
            lo = [int(rs.randint(1, max(2, n // 3))) for n in bs]
            seg[tuple(slice(l, l + max(2, n // 3)) for l, n in zip(lo, bs))] = label
        full = np.zeros(c['shape'], dtype=np.int16)
        full[body] = seg
        img[body] += 150.0 * (seg > 0)
        img[body][img[body] == 0] = 1
        geo = dict(spacing=c['spacing'][::-1], origin=(-12.5, 8.0, 30.25))
        write_image(img, os.path.join(folder, 'imagesTr', c['id'] + '_0000.nii.gz'), **geo)
        write_image(full.astype(c['seg_dtype']), os.path.join(folder, 'labelsTr', c['id'] + '.nii.gz'), **geo)
    names = ['background'] + ['structure_%d' % i for i in range(1, task['labels'])]
    with open(os.path.join(folder, 'dataset.json'), 'w') as f:
        json.dump({'name': task['name'], 'modality': {'0': task['modality']}, 'labels': {str(i): n for i, n in enumerate(names)},
                   'numTraining': len(task['cases']), 'numTest': 0, 'test': [],
                   'training': [{'image': './imagesTr/%s.nii.gz' % c['id'], 'label': './labelsTr/%s.nii.gz' % c['id']}
                                for c in task['cases']]}, f)
    return folder


class ToyEnvironment(object):
    """The three folders of the reference's environment variables under `root`, set for as long as the object lives (a module
    fixture closes it).  `plan_and_preprocess(task, *argv)` writes the toy task when it is not there yet and runs the driver."""

    def __init__(self, root):
        import pytest
        self.root = str(root)
        self.mp = pytest.MonkeyPatch()
        self.base = os.path.join(self.root, 'base')
        self.raw = os.path.join(self.base, 'nnUNet_raw_data')
        self.cropped = os.path.join(self.base, 'nnUNet_cropped_data')
        self.preprocessed = os.path.join(self.root, 'preprocessed')
        self.results = os.path.join(self.root, 'results')
        for d in (self.raw, self.preprocessed, self.results):
            os.makedirs(d)
        self.mp.setenv('nnUNet_raw_data_base', self.base)
        self.mp.setenv('nnUNet_preprocessed', self.preprocessed)
        self.mp.setenv('RESULTS_FOLDER', self.results)

    def close(self):
        self.mp.undo()

    def plan_and_preprocess(self, task, *argv):
        from multitalent_amd.experiment_planning.nnUNet_plan_and_preprocess import main
        if not os.path.isdir(os.path.join(self.raw, task['name'])):
            write_toy_task(self.raw, task)
        main(['-t', task['name'][4:7], '-pl2d', 'None', '-tf', '2', '-tl', '2'] + list(argv))


def load_pickle(fname):
    with open(fname, 'rb') as f:
        return pickle.load(f)


def load_cases(folder):
    """{case: (array of <case>.npz, properties of <case>.pkl)} of a cropped or preprocessed folder."""
    return OrderedDict((f[:-4], (np.load(os.path.join(folder, f))['data'], load_pickle(os.path.join(folder, f[:-4] + '.pkl'))))
                       for f in sorted(os.listdir(folder)) if f.endswith('.npz'))


def assert_same_cases(got, want, ignore=()):
    """Arrays bit for bit (dtype, shape, bytes), properties equal in the codec (minus the keys of `ignore`)."""
    assert list(got) == list(want)
    for k in want:
        (a, pa), (b, pb) = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        assert encode({i: v for i, v in pa.items() if i not in ignore}) == encode({i: v for i, v in pb.items() if i not in ignore}), k


def expected_shape(properties, target_spacing, transpose_forward):
    """round(original_spacing / target * shape) of a cropped case, in transposed order."""
    sp = np.array(properties['original_spacing'])[transpose_forward]
    return tuple(int(i) for i in np.round(sp / np.array(target_spacing) * np.array(properties['size_after_cropping'])[transpose_forward]))
