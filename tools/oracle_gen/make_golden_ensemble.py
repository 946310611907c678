"""Golden vectors for the stock prediction / ensembling drivers: the REAL reference run on CPU in the build container.

(a) `nnunet.inference.ensemble_predictions.merge` (:56-95, `merge_files` :26-53 underneath) on three member folders of three
    synthetic cases (12x20x24, an odd 11x19x23, and a 10x14x18 case whose pkls carry `regions_class_order`), C = 3, crop box strictly
    inside a larger original volume, with `store_npz=True` and a postprocessing file.
(b) `nnunet.evaluation.model_selection.ensemble.merge` (:26-36) on two of those members.
(c) `nnunet.inference.predict.predict_cases` (:131-291) with a tiny `nnUNetTrainerV2` softmax model of two folds, `save_npz=True`
    and a `postprocessing.json` in the model folder; `nnunet.postprocessing.consolidate_postprocessing.consolidate_folds` (:43-85)
    over synthetic `fold_*/validation_raw` folders.

The members are float16 values chosen for the arithmetic of the merge: smooth softmax-like regions, exact zeros, float16
subnormals, values quantised to 1/8 (so that float16-equal means and means of exactly 0.5 occur).  The number of voxels whose two
largest reference means are EQUAL is recorded and asserted to be above zero; for the `predict_cases` case the number of voxels
within 1e-4 of a decision boundary (tests/mask_check.py's rule, on the reference's float32 probabilities) is recorded and asserted
to be at most 1 % of the voxels.  The raw case of (c) has the plan's spacing, so neither side resamples.

Substitutions for what this image lacks, all at third-party seams (the same as make_golden_drivers / make_golden_postprocessing):
  * SimpleITK -> a shim over multitalent_amd.utilities.nifti_io (real .nii.gz files on disk);
  * skimage.transform.resize -> scipy.ndimage.zoom(mode='nearest', grid_mode=True); batchgenerators' file helpers -> restatements;
  * multiprocessing Pool -> a synchronous stand-in (starmap / starmap_async / map);
  * the reference's `aggregate_scores` (SimpleITK + pandas + medpy underneath) -> multitalent_amd.evaluation.evaluator.aggregate_scores
    on its host path, the seam make_golden_postprocessing uses: the Dice values of (c) are therefore the reference's
    `consolidate_folds` and `determine_postprocessing` over that scorer.

Writes tests/golden/ensemble.npz and tests/golden/ensemble.json.  Run: python tools/oracle_gen/make_golden_ensemble.py"""
import json
import os
import pickle
import shutil
import sys
import tempfile
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_import
ref_import.install()

from multitalent_amd.utilities import nifti_io                                    # the shim's backend (file format only)
from multitalent_amd.evaluation.evaluator import aggregate_scores

nifti_io._have_sitk = lambda: False          # the import shim makes `import SimpleITK` succeed: use the NIfTI codec itself

import batchgenerators.utilities.file_and_folder_operations as ffo


def _save_json(obj, file, indent=4, sort_keys=True):
    with open(file, 'w') as f:
        json.dump(obj, f, sort_keys=sort_keys, indent=indent)


def _load_json(file):
    with open(file) as f:
        return json.load(f)


def _subfolders(folder, join=True, prefix=None, suffix=None, sort=True):
    r = [os.path.join(folder, i) if join else i for i in os.listdir(folder) if os.path.isdir(os.path.join(folder, i))
         and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
    return sorted(r) if sort else r


def _subfiles(folder, join=True, prefix=None, suffix=None, sort=True):
    r = [os.path.join(folder, i) if join else i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i))
         and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
    return sorted(r) if sort else r


def _save_pickle(obj, file, mode='wb'):
    with open(file, mode) as f:
        pickle.dump(obj, f)


FFO = {'save_json': _save_json, 'load_json': _load_json, 'subfolders': _subfolders, 'subfiles': _subfiles, 'save_pickle': _save_pickle,
       'subdirs': _subfolders, 'write_pickle': _save_pickle}
for n, f in FFO.items():
    setattr(ffo, n, f)
ffo.__all__ = list(ffo.__all__) + list(FFO)
FFO_NAMES = list(FFO) + ['join', 'isfile', 'isdir', 'maybe_mkdir_p', 'load_pickle']


class _SitkImage:
    def __init__(self, arr):
        self.arr = np.asarray(arr)
        self.spacing, self.origin, self.direction = (1., 1., 1.), (0., 0., 0.), tuple(np.eye(3).ravel())

    def SetSpacing(self, s): self.spacing = tuple(s)
    def SetOrigin(self, s): self.origin = tuple(s)
    def SetDirection(self, s): self.direction = tuple(s)
    def GetSpacing(self): return self.spacing
    def GetOrigin(self): return self.origin
    def GetDirection(self): return self.direction
    def GetSize(self): return tuple(int(i) for i in self.arr.shape[::-1])


def _read(fname):
    im = nifti_io._read_nifti(fname)
    o = _SitkImage(im.array)
    o.spacing, o.origin, o.direction = im.spacing, im.origin, im.direction
    return o


SITK = SimpleNamespace(GetImageFromArray=lambda a: _SitkImage(a), GetArrayFromImage=lambda im: im.arr, ReadImage=_read,
                       WriteImage=lambda im, f: nifti_io._write_nifti(nifti_io.Image(im.arr, im.spacing, im.origin, im.direction), f))


class _SyncResult:
    def __init__(self, v): self.v = v
    def get(self): return self.v


class _SyncPool:
    def __init__(self, *a, **k): pass
    def starmap(self, fn, args): return [fn(*a) for a in args]
    def starmap_async(self, fn, args): return _SyncResult([fn(*a) for a in args])
    def map(self, fn, args): return [fn(a) for a in args]
    def close(self): pass
    def join(self): pass


def _resize(img, shape, order, mode='edge', anti_aliasing=False, **kw):
    assert mode == 'edge' and not anti_aliasing
    img = np.asarray(img, dtype=float)
    return ndimage.zoom(img, [n / o for n, o in zip(shape, img.shape)], order=order, mode='nearest', grid_mode=True)


def _resize_segmentation(segmentation, new_shape, order=3):
    if order == 0:
        return _resize(segmentation.astype(float), new_shape, 0).astype(segmentation.dtype)
    out = np.zeros(new_shape, dtype=segmentation.dtype)
    for c in np.unique(segmentation):
        out[_resize((segmentation == c).astype(float), new_shape, order) >= 0.5] = c
    return out


import nnunet.preprocessing.preprocessing as pre
import nnunet.preprocessing.cropping as crop
import nnunet.inference.segmentation_export as se
import nnunet.utilities.sitk_stuff as sitk_stuff
import nnunet.postprocessing.connected_components as cc
import nnunet.postprocessing.consolidate_postprocessing as cons
import nnunet.inference.ensemble_predictions as ens
import nnunet.evaluation.model_selection.ensemble as msel
import nnunet.inference.predict as pred
import nnunet.training.model_restore as mr
import nnunet.training.network_training.nnUNetTrainer as nt
import nnunet.training.network_training.network_trainer as nwt
import nnunet.training.network_training.nnUNetTrainerV2 as v2

pre.resize = _resize
pre.resize_segmentation = _resize_segmentation
for m in (crop, se, sitk_stuff, cc, pred):
    m.sitk = SITK
for m in (cc, ens, msel, pred):
    m.Pool = _SyncPool
cc.aggregate_scores = aggregate_scores
cons.aggregate_scores = aggregate_scores
for m in (pre, crop, se, cc, cons, ens, msel, pred, mr, nt, nwt, v2):
    for n in FFO_NAMES:
        setattr(m, n, getattr(ffo, n))
# the loader's oversized patch (batchgenerators' rotate_coords_3d, absent) plays no role in prediction
v2.get_patch_size = lambda final_patch_size, *a, **k: np.array(final_patch_size)
_real_torch_load = torch.load
torch.load = lambda f, map_location=None, **k: _real_torch_load(f, map_location=map_location, weights_only=False)

OUT = os.path.join(ROOT, 'tests', 'golden')
IP = {0: {'mean': 63.44, 'sd': 175.48, 'percentile_00_5': -927.0, 'percentile_99_5': 275.0}}
STAGE = {'batch_size': 2, 'patch_size': np.array([8, 16, 16]), 'pool_op_kernel_sizes': [[2, 2, 2], [1, 2, 2]],
         'conv_kernel_sizes': [[3, 3, 3]] * 3, 'do_dummy_2D_data_aug': False, 'current_spacing': np.array([2.0, 1.0, 1.0]),
         'num_pool_per_axis': [1, 2, 2]}
C = 3
SEED = 57                     # of the network weights of (c): all three classes occur in the prediction
FOLDERS = ('m0', 'm1', 'm2')
# name, box, original volume, lower corner of the box, regions_class_order
CASES = (('caseA', (12, 20, 24), (15, 26, 27), (2, 3, 1), None),
         ('caseB', (11, 19, 23), (13, 21, 29), (1, 1, 4), None),
         ('caseR', (10, 14, 18), (12, 15, 21), (1, 1, 2), [2, 3, 1]))
SPACING, ORIGIN = (2.5, 0.75, 0.75), (-3.5, 12.0, 40.25)           # of the member cases (z, y, x spacing; itk origin)
PP_MERGE = {'for_which_classes': [1, 2], 'min_valid_object_sizes': '{1: 40.0, 2: 25.0}'}
PP_MODEL = {'for_which_classes': [1, [1, 2]]}


def member(rng, shape, kind):
    """One member's float16 probabilities [C, *shape].  `kind` [*shape] in 0..3 picks what a voxel holds (the same for every member
    of a case, so that the special values meet each other in the mean)."""
    logits = np.stack([ndimage.gaussian_filter(rng.standard_normal(shape), 1.5) for _ in range(C)]) * 12
    e = np.exp(logits - logits.max(0))
    p = (e / e.sum(0)).astype(np.float16)                                             # 0: softmax-like, smooth
    q = (rng.integers(0, 9, (C,) + shape) / 8.0).astype(np.float16)                    # 1: multiples of 1/8 (0.5 among them)
    sub = rng.integers(0, 1024, (C,) + shape).astype(np.uint16).view(np.float16)       # 2: float16 subnormals (and zero) ...
    big = rng.integers(0, C, shape)
    for c in range(C):
        sub[c][big == c] = np.float16(1.0) - np.float16(rng.integers(0, 3) / 1024.0)   # ... beside one channel near 1
    z = np.where(rng.random((C,) + shape) < 0.6, 0.0, q).astype(np.float16)            # 3: mostly exact zeros
    out = np.where(kind[None] == 0, p, np.where(kind[None] == 1, q, np.where(kind[None] == 2, sub, z)))
    return np.ascontiguousarray(out.astype(np.float16))


def case_properties(name, shape, full, lo, order):
    sp = SPACING
    p = OrderedDict(list_of_data_files=['/raw/imagesTs/' + name + '_0000.nii.gz'], original_spacing=np.array(sp),
                    spacing_after_resampling=np.array(sp), size_after_cropping=np.array(shape),
                    original_size_of_raw_data=np.array(full), crop_bbox=[[lo[i], lo[i] + shape[i]] for i in range(3)],
                    itk_spacing=tuple(sp[::-1]), itk_origin=ORIGIN, itk_direction=tuple(np.eye(3).ravel()))
    if order is not None:
        p['regions_class_order'] = list(order)
    return p


def read_seg(f):
    return nifti_io._read_nifti(f).array.astype(np.uint8)


def part_a_b(tmp, rec, meta):
    rng = np.random.default_rng(20261018)
    for f in FOLDERS:
        os.makedirs(os.path.join(tmp, f))
    equal_top2 = 0
    for name, shape, full, lo, order in CASES:
        kind = rng.choice(4, size=shape, p=[0.5, 0.25, 0.15, 0.10])
        for f in FOLDERS:
            m = member(rng, shape, kind)
            np.savez_compressed(os.path.join(tmp, f, name + '.npz'), softmax=m)
            _save_pickle(case_properties(name, shape, full, lo, order), os.path.join(tmp, f, name + '.pkl'))
            rec['a/%s/%s' % (f, name)] = m
    pp = os.path.join(tmp, 'pp_merge.json')
    _save_json(PP_MERGE, pp)
    out = os.path.join(tmp, 'merged')
    ens.merge([os.path.join(tmp, f) for f in FOLDERS], out, 2, override=True, postprocessing_file=pp, store_npz=True)
    assert os.path.isfile(os.path.join(out, 'pp_merge.json'))
    for name, shape, full, lo, order in CASES:
        raw = os.path.join(out, 'not_postprocessed', name)
        mean = np.load(raw + '.npz')['softmax']
        assert mean.dtype == np.float16 and mean.shape == (C,) + shape
        props = pickle.load(open(raw + '.pkl', 'rb'))
        assert isinstance(props, list) and len(props) == len(FOLDERS)
        rec['a/merged/%s/mean' % name] = mean
        rec['a/merged/%s/seg' % name] = read_seg(raw + '.nii.gz')
        rec['a/merged/%s/seg_pp' % name] = read_seg(os.path.join(out, name + '.nii.gz'))
        assert rec['a/merged/%s/seg' % name].shape == full
        srt = np.sort(mean.astype(np.float32), 0)
        eq = int((srt[-1] == srt[-2]).sum())
        half = int((mean == np.float16(0.5)).sum())
        subn = int(((mean != 0) & (np.abs(mean.astype(np.float32)) < 2.0 ** -14)).sum())
        meta['a']['cases'][name] = {'shape': list(shape), 'full': list(full), 'lo': list(lo), 'regions_class_order': order,
                                    'equal_top2': eq, 'means_exactly_half': half, 'subnormal_means': subn,
                                    'differs_after_pp': int((rec['a/merged/%s/seg' % name] != rec['a/merged/%s/seg_pp' % name]).sum())}
        equal_top2 += eq
        print('merge', name, 'labels', np.bincount(rec['a/merged/%s/seg' % name].ravel()), meta['a']['cases'][name])
    meta['a']['equal_top2'] = equal_top2
    assert equal_top2 > 0, "the members must produce float16-equal top-two means"
    assert all(v['means_exactly_half'] > 0 and v['subnormal_means'] > 0 for v in meta['a']['cases'].values())
    # (b) model_selection.ensemble.merge on members m0 and m2 (argmax whatever the pkl says, :35)
    for name, shape, full, lo, order in CASES:
        o = os.path.join(tmp, 'msel_' + name + '.nii.gz')
        msel.merge((os.path.join(tmp, 'm0', name + '.npz'), os.path.join(tmp, 'm2', name + '.npz'), os.path.join(tmp, 'm0', name + '.pkl'), o))
        rec['b/%s/seg' % name] = read_seg(o)


def make_plans():
    return {'num_stages': 2, 'num_modalities': 1, 'modalities': {0: 'CT'}, 'normalization_schemes': OrderedDict({0: 'CT'}),
            'num_classes': C - 1, 'all_classes': list(range(1, C)), 'base_num_features': 4, 'use_mask_for_norm': OrderedDict({0: False}),
            'transpose_forward': [0, 1, 2], 'transpose_backward': [0, 1, 2], 'data_identifier': 'nnUNetData_plans_v2.1',
            'conv_per_stage': 2, 'plans_per_stage': {1: dict(STAGE)}, 'preprocessor_name': 'GenericPreprocessor',
            'dataset_properties': {'intensityproperties': IP}, 'keep_only_largest_region': None, 'min_region_size_per_class': None,
            'min_size_per_class': None}


def randomize(net, seed):
    g = torch.Generator().manual_seed(seed)
    for n, p in net.named_parameters():
        if p.dim() == 1 and ('norm' in n) and n.endswith('weight'):
            p.data = 0.5 + torch.rand(p.shape, generator=g)
        elif n.endswith('bias'):
            p.data = 0.3 * torch.randn(p.shape, generator=g)
        elif 'seg_outputs' in n:
            p.data = 4.0 * torch.randn(p.shape, generator=g)       # lively heads: confident, varied classes, few near-ties


def ct_volume(rs, shape):
    v = ndimage.gaussian_filter(rs.randn(*shape), 1.2) * 700 + 40
    v[:2] = 0; v[:, :1] = 0; v[:, :, -2:] = 0                  # a zero border: crop_to_nonzero has something to cut
    return v.astype(np.float32)


def part_c_predict(tmp, rec, meta):
    torch.manual_seed(SEED)                                   # the body's He initialisation
    plans = make_plans()
    model = os.path.join(tmp, 'res', 'nnUNet', '3d_fullres', 'Task555_Tiny', 'nnUNetTrainerV2__nnUNetPlansv2.1')
    os.makedirs(model)
    plans_file = os.path.join(tmp, 'plans_3D.pkl')
    _save_pickle(plans, plans_file)
    _save_pickle(plans, os.path.join(model, 'plans.pkl'))
    base_sd = None
    for fold in (0, 1):
        tr = v2.nnUNetTrainerV2(plans_file, fold, output_folder=model, dataset_directory=os.path.join(tmp, 'pre'), batch_dice=True, stage=1,
                                unpack_data=False, deterministic=False, fp16=False)
        tr.initialize(False)
        if base_sd is not None:
            tr.network.load_state_dict(base_sd)                 # the folds share the body and differ in norms, biases and heads
        randomize(tr.network, SEED + fold)
        sd = {k: v.detach().cpu().numpy().copy() for k, v in tr.network.state_dict().items()}
        if base_sd is None:
            base_sd = {k: v.clone() for k, v in tr.network.state_dict().items()}
            for k, v in sd.items():
                rec['c/sd0/' + k] = v
        else:
            for k, v in sd.items():
                if not np.array_equal(v, rec['c/sd0/' + k]):
                    rec['c/sd1/' + k] = v
        tr.epoch = 4
        tr.lr_scheduler = None
        tr.optimizer = SimpleNamespace(state_dict=lambda: {})
        tr.amp_grad_scaler = None
        assert tr.output_folder.endswith('fold_%d' % fold)
        tr.save_checkpoint(os.path.join(tr.output_folder, 'model_final_checkpoint.model'))
    _save_json(PP_MODEL, os.path.join(model, 'postprocessing.json'))
    inp, outp = os.path.join(tmp, 'in'), os.path.join(tmp, 'out')
    os.makedirs(inp)
    rs = np.random.RandomState(11)
    name, shape, sp = 'caseP', (14, 27, 25), (2.0, 1.0, 1.0)           # the plan's spacing: no resampling on either side
    v = ct_volume(rs, shape)
    origin = (-12.5, 30.0, 7.25)
    nifti_io._write_nifti(nifti_io.Image(v, sp[::-1], origin, tuple(np.eye(3).ravel())), os.path.join(inp, name + '_0000.nii.gz'))
    rec['c/raw/vol'] = v
    captured = {}
    real_save = pred.save_segmentation_nifti_from_softmax

    def capture(softmax, out_fname, *a, **k):
        captured['probs'] = np.array(softmax, dtype=np.float32, copy=True)
        real_save(softmax, out_fname, *a, **k)
        captured['seg'] = read_seg(out_fname)                   # before load_remove_save overwrites the file

    pred.save_segmentation_nifti_from_softmax = capture
    pred.predict_cases(model, [[os.path.join(inp, name + '_0000.nii.gz')]], [os.path.join(outp, name + '.nii.gz')], [0, 1], True, 1, 1,
                       None, True, mixed_precision=False, overwrite_existing=True, all_in_gpu=False, step_size=0.5,
                       checkpoint_name='model_final_checkpoint')
    pred.save_segmentation_nifti_from_softmax = real_save
    assert os.path.isfile(os.path.join(outp, 'postprocessing.json'))
    probs = captured['probs']
    stored = np.load(os.path.join(outp, name + '.npz'))['softmax']
    props = pickle.load(open(os.path.join(outp, name + '.pkl'), 'rb'))
    assert stored.dtype == np.float16 and stored.shape == probs.shape
    assert tuple(props['size_after_cropping']) == probs.shape[1:], "the case must not be resampled"
    srt = np.sort(probs, 0)
    ties = int(((srt[-1] - srt[-2]) <= 1e-4).sum())
    nvox = int(np.prod(probs.shape[1:]))
    assert ties <= 0.01 * nvox, "%d of %d voxels within 1e-4 of a decision boundary: choose other inputs" % (ties, nvox)
    rec['c/probs'] = probs
    rec['c/npz'] = stored
    rec['c/seg'] = captured['seg']
    rec['c/seg_pp'] = read_seg(os.path.join(outp, name + '.nii.gz'))
    assert rec['c/seg'].shape == shape
    meta['c']['predict'] = {'case': name, 'shape': list(shape), 'spacing_zyx': list(sp), 'origin': list(origin), 'voxels': nvox,
                            'ties_1e-4': ties, 'crop_bbox': [[int(j) for j in i] for i in props['crop_bbox']],
                            'size_after_cropping': [int(i) for i in props['size_after_cropping']],
                            'postprocessing': PP_MODEL, 'intensityproperties': IP[0],
                            'differs_after_pp': int((rec['c/seg'] != rec['c/seg_pp']).sum())}
    print('predict_cases', name, probs.shape, 'labels', np.bincount(rec['c/seg'].ravel()), meta['c']['predict'])


def blob(shape, centre, radii):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2 <= 1


def part_c_consolidate(tmp, rec, meta):
    base = os.path.join(tmp, 'cv')
    s, sp = (16, 24, 24), (1.5, 0.8, 0.8)
    names = {0: ['cv0', 'cv1'], 1: ['cv2', 'cv3']}
    k = 0
    for fold, cases in names.items():
        vf = os.path.join(base, 'fold_%d' % fold, 'validation_raw')
        os.makedirs(vf)
        os.makedirs(os.path.join(base, 'gt_niftis'), exist_ok=True)
        pairs = []
        for cname in cases:
            gt = np.zeros(s, np.uint8)
            c = (8 + k % 2, 12, 11 + k)
            gt[blob(s, c, (6, 8, 8))] = 2
            gt[blob(s, c, (3, 4, 4))] = 1
            raw = gt.copy()
            raw[blob(s, c, (6, 8, 9))] = 2
            raw[blob(s, c, (3, 4, 4))] = 1
            raw[:, :, :2] = 0
            raw[0:2, 0:2, 20:22] = 1                          # spurious specks of both classes, away from the object
            raw[13:15, 20:23, 20:23] = 2
            raw[14:16, 0:3 + k % 2, 0:2] = 2
            for folder, arr in ((vf, raw), (os.path.join(base, 'gt_niftis'), gt)):
                nifti_io._write_nifti(nifti_io.Image(arr, sp[::-1], (0., 0., 0.), tuple(np.eye(3).ravel())), os.path.join(folder, cname + '.nii.gz'))
            rec['c/cv/%d/%s/raw' % (fold, cname)] = raw
            rec['c/cv/%d/%s/gt' % (fold, cname)] = gt
            pairs.append((os.path.join(vf, cname + '.nii.gz'), os.path.join(base, 'gt_niftis', cname + '.nii.gz')))
            k += 1
        aggregate_scores(pairs, labels=[0, 1, 2], json_output_file=os.path.join(vf, 'summary.json'))
    cons.consolidate_folds(base, folds=(0, 1))
    pp = _load_json(os.path.join(base, 'postprocessing.json'))
    dice = {}
    for sub in ('cv_niftis_raw', 'cv_niftis_postprocessed'):
        mean = _load_json(os.path.join(base, sub, 'summary.json'))['results']['mean']
        dice[sub] = {c: mean[c]['Dice'] for c in sorted(mean)}
    for cases in names.values():
        for cname in cases:
            rec['c/cv/final/' + cname] = read_seg(os.path.join(base, 'cv_niftis_postprocessed', cname + '.nii.gz'))
    meta['c']['consolidate'] = {'spacing_zyx': list(sp), 'folds': {str(f): c for f, c in names.items()}, 'postprocessing': pp, 'dice': dice,
                                'folders': sorted(os.listdir(base))}
    print('consolidate_folds', pp['for_which_classes'], pp.get('min_valid_object_sizes'), dice)


def main():
    torch.set_num_threads(8)
    tmp = tempfile.mkdtemp(prefix='mt_golden_ensemble_')
    rec, meta = {}, {'a': {'folders': list(FOLDERS), 'spacing_zyx': list(SPACING), 'origin': list(ORIGIN), 'postprocessing': PP_MERGE, 'cases': {}}, 'b': {'members': ['m0', 'm2']}, 'c': {}}
    try:
        part_a_b(tmp, rec, meta)
        part_c_predict(tmp, rec, meta)
        part_c_consolidate(tmp, rec, meta)
        dst = os.path.join(OUT, 'ensemble.npz')
        np.savez_compressed(dst, **rec)
        with open(os.path.join(OUT, 'ensemble.json'), 'w') as f:
            json.dump(meta, f, indent=1, sort_keys=True)
        print('wrote', dst, os.path.getsize(dst) // 1024, 'KiB')
        assert os.path.getsize(dst) < 1024 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
