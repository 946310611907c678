"""Golden vectors for the connected-component postprocessing: the REAL reference's
nnunet/postprocessing/connected_components.py run on CPU in the build container on small synthetic label volumes.

(a) `remove_all_but_the_largest_connected_component` (:48-101) on seeded 24-40 voxel volumes with 3-4 labels: for_which_classes
    None, a list of ints, a tuple entry followed by one of its members, a dict of minimum sizes, two components tied for the
    largest, an anisotropic volume_per_voxel.  Output images and both dicts are recorded.
(b) `determine_postprocessing` (:119-397) on synthetic `validation_raw/` + `gt_segmentations/` folders: the all-foreground removal
    accepted; rejected with the per-class step keeping a subset; a single-class dataset; advanced_postprocessing=True.
    postprocessing.json and the validation_final masks are recorded.

Substitutions for what this image lacks, all at third-party seams:
  * SimpleITK -> a shim over multitalent_amd.utilities.nifti_io (real .nii.gz files on disk, read and written by it);
  * batchgenerators' file helpers (load_json, save_json, subfiles, maybe_mkdir_p) -> plain restatements;
  * multiprocessing Pool -> a synchronous stand-in with the same starmap_async(...).get() surface;
  * the reference's `aggregate_scores` (SimpleITK + pandas + medpy underneath) -> the repository's
    multitalent_amd.evaluation.evaluator.aggregate_scores, the same seam the product uses.
Under numpy >= 2 the reference's str() of its np.float64 sizes reads "np.float64(x)" in `min_valid_object_sizes`; the string is
recorded as the reference wrote it.

Writes tests/golden/postprocessing.npz (uint8 volumes) and tests/golden/postprocessing.json.
Run: python tools/oracle_gen/make_golden_postprocessing.py"""
import json
import os
import shutil
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_import
ref_import.install()

from multitalent_amd.utilities import nifti_io                                    # the shim's backend (file format only)
from multitalent_amd.evaluation.evaluator import aggregate_scores

nifti_io._have_sitk = lambda: False          # the import shim makes `import SimpleITK` succeed: use the NIfTI codec itself


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
    def starmap_async(self, fn, args): return _SyncResult([fn(*a) for a in args])
    def close(self): pass
    def join(self): pass


def _load_json(f):
    with open(f) as fh:
        return json.load(fh)


def _save_json(obj, f, indent=4, sort_keys=True):
    with open(f, 'w') as fh:
        json.dump(obj, fh, sort_keys=sort_keys, indent=indent)


def _subfiles(folder, join=True, prefix=None, suffix=None, sort=True):
    r = [os.path.join(folder, i) if join else i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i))
         and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
    return sorted(r) if sort else r


import nnunet.utilities.sitk_stuff as sitk_stuff
import nnunet.postprocessing.connected_components as cc

sitk_stuff.sitk = SITK
cc.sitk = SITK
cc.Pool = _SyncPool
cc.aggregate_scores = aggregate_scores
cc.load_json, cc.save_json, cc.subfiles = _load_json, _save_json, _subfiles
cc.join, cc.isdir, cc.isfile = os.path.join, os.path.isdir, os.path.isfile
cc.maybe_mkdir_p = lambda p: os.makedirs(p, exist_ok=True)


def blob(shape, centre, radii):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2 <= 1


def specks(rng, img, label, n, size=2):
    for _ in range(n):
        c = [int(rng.integers(0, s - size)) for s in img.shape]
        img[c[0]:c[0] + size, c[1]:c[1] + int(rng.integers(1, size + 1)), c[2]:c[2] + size] = label


def volumes_a():
    """(name, image, for_which_classes, volume_per_voxel, minimum_valid_object_size)"""
    rng = np.random.default_rng(20261016)
    out = []
    s = (28, 36, 40)
    img = np.zeros(s, np.uint8)
    img[blob(s, (14, 12, 12), (8, 9, 9))] = 1
    img[blob(s, (14, 24, 28), (7, 8, 8))] = 2
    img[blob(s, (6, 28, 10), (4, 5, 5))] = 3
    specks(rng, img, 1, 12); specks(rng, img, 2, 10); specks(rng, img, 3, 8, 3)
    out.append(('none', img.copy(), None, 1.0, None))
    out.append(('list_aniso', img.copy(), [1, 3], 0.7 * 0.7 * 2.5, None))
    img2 = img.copy()
    img2[blob(s, (20, 12, 30), (4, 6, 6))] = 2            # a class-2 object touching nothing of class 1
    img2[blob(s, (9, 12, 24), (3, 4, 4))] = 2              # a class-2 object touching the class-1 blob
    out.append(('tuple_then_member', img2, [(1, 2), 1], 0.5, None))
    out.append(('min_sizes', img.copy(), [1, 2, 3], 1.3, {1: 5.0, 2: 11.0, 3: 30.0}))
    s = (24, 32, 32)
    img = np.zeros(s, np.uint8)
    img[2:6, 2:6, 2:6] = 1                                  # 64 voxels
    img[10:14, 20:24, 20:24] = 1                            # 64 voxels: tied for the largest
    img[18:20, 2:4, 2:4] = 1                                # 8 voxels
    img[2:8, 20:30, 2:8] = 4
    img[15:22, 3:9, 22:30] = 4
    specks(rng, img, 4, 6)
    out.append(('tie', img, [1, 4], 0.9 * 0.9 * 1.5, None))
    img = (rng.random((24, 26, 30)) < 0.3116).astype(np.uint8) * rng.integers(1, 4, (24, 26, 30)).astype(np.uint8)
    out.append(('random_three_labels', img, [1, 2, (2, 3), 3], 2.0, None))
    return out


def keyrepr(d):
    """dict -> [[repr(key), value]]; numpy integer keys (for_which_classes=None iterates np.unique) are written as ints"""
    return None if d is None else [[repr(int(k) if isinstance(k, np.integer) else k), v] for k, v in d.items()]


def write_case(folder, name, arr, spacing):
    os.makedirs(folder, exist_ok=True)
    nifti_io._write_nifti(nifti_io.Image(arr, spacing, (1.5, -2.0, 3.0), tuple(np.eye(3).ravel())), os.path.join(folder, name + '.nii.gz'))


def scenarios_b():
    """(name, labels incl. 0, advanced, cases: [(case name, raw, gt, spacing)])"""
    rng = np.random.default_rng(7)
    s = (24, 32, 32)
    res = []
    # 1. the all-foreground removal helps every class: class 1 core inside a class 2 shell, spurious specks of both elsewhere
    cases = []
    for k in range(3):
        gt = np.zeros(s, np.uint8)
        c = (12 + k, 16, 15 + k)
        gt[blob(s, c, (8, 10, 10))] = 2
        gt[blob(s, c, (4, 5, 5))] = 1
        raw = gt.copy()
        raw[blob(s, c, (8, 10, 11))] = 2
        raw[blob(s, c, (4, 5, 5))] = 1
        raw[:, :, :3] = 0
        raw[0:2, 0:2, 28:30] = 1
        raw[20:22, 28:30, 28:31] = 2
        raw[22:24, 0:3, 0:2] = 2
        cases.append(('case%d' % k, raw, gt, (0.8, 0.8, 2.0)))
    res.append(('fg_accepted', [0, 1, 2], False, cases))
    # 2. rejected (the class-1 object is separate from the larger class-2 object), per-class keeps class 1 only
    cases = []
    for k in range(3):
        gt = np.zeros(s, np.uint8)
        gt[blob(s, (7, 9, 9), (4, 5, 5))] = 1
        gt[blob(s, (15, 22, 22), (6, 8, 8))] = 2
        gt[blob(s, (18, 6, 26), (3, 3, 3))] = 2                       # a true second class-2 object
        raw = gt.copy()
        raw[20:22, 2 + k:4 + k, 2:4] = 1                              # a spurious class-1 speck
        raw[blob(s, (7, 9, 9), (4, 5, 4))] = 1
        cases.append(('case%d' % k, raw, gt, (1.0, 0.7, 0.7)))
    res.append(('fg_rejected_per_class', [0, 1, 2], False, cases))
    # 3. one class
    cases = []
    for k in range(2):
        gt = np.zeros(s, np.uint8)
        gt[blob(s, (12, 16, 16), (7, 9, 9))] = 1
        raw = gt.copy()
        specks(rng, raw, 1, 5)
        cases.append(('case%d' % k, raw, gt, (1.5, 1.0, 1.0)))
    res.append(('single_class', [0, 1], False, cases))
    # 4. advanced: the scenario-2 volumes plus scattered specks of every class
    cases = []
    for name, raw, gt, sp in res[1][3]:
        raw = raw.copy()
        specks(rng, raw, 1, 3); specks(rng, raw, 2, 3)
        cases.append((name, raw, gt, sp))
    res.append(('advanced', [0, 1, 2], True, cases))
    return res


def main():
    arrays, meta = {}, {'a': [], 'b': []}
    for name, img, fwc, vpv, mins in volumes_a():
        arrays['a/%s/in' % name] = img.copy()
        out, lr, ks = cc.remove_all_but_the_largest_connected_component(img.copy(), fwc, vpv, mins)
        arrays['a/%s/out' % name] = out
        meta['a'].append(dict(name=name, for_which_classes=repr(fwc), volume_per_voxel=vpv, min_sizes=repr(mins),
                              largest_removed=keyrepr({k: float(v) if v is not None else None for k, v in lr.items()}),
                              kept_size=keyrepr({k: float(v) if v is not None else None for k, v in ks.items()})))
        print(name, lr, ks)
    for name, labels, adv, cases in scenarios_b():
        base = tempfile.mkdtemp()
        try:
            for cname, raw, gt, sp in cases:
                write_case(os.path.join(base, 'validation_raw'), cname, raw, sp)
                write_case(os.path.join(base, 'gt_segmentations'), cname, gt, sp)
                arrays['b/%s/%s/raw' % (name, cname)] = raw
                arrays['b/%s/%s/gt' % (name, cname)] = gt
                arrays['b/%s/%s/spacing' % (name, cname)] = np.array(sp, np.float64)
            aggregate_scores([[os.path.join(base, 'validation_raw', c + '.nii.gz'), os.path.join(base, 'gt_segmentations', c + '.nii.gz')]
                              for c, _, _, _ in cases], labels=labels, json_output_file=os.path.join(base, 'validation_raw', 'summary.json'))
            cc.determine_postprocessing(base, os.path.join(base, 'gt_segmentations'), 'validation_raw', final_subf_name='validation_final',
                                        advanced_postprocessing=adv)
            pp = _load_json(os.path.join(base, 'postprocessing.json'))
            for cname, _, _, _ in cases:
                arrays['b/%s/%s/final' % (name, cname)] = nifti_io._read_nifti(os.path.join(base, 'validation_final', cname + '.nii.gz')).array
            left = sorted(os.listdir(base))
            meta['b'].append(dict(name=name, labels=labels, advanced=adv, cases=[c[0] for c in cases], postprocessing=pp, folders=left))
            print(name, pp['for_which_classes'], pp['min_valid_object_sizes'], left)
        finally:
            shutil.rmtree(base)
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'postprocessing.npz'), **arrays)
    with open(os.path.join(ROOT, 'tests', 'golden', 'postprocessing.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
