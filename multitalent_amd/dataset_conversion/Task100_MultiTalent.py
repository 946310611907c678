"""Task100_MultiTalent: the region tables (loss semantics of the hot path) and the dataset conversion that merges the 13 source
tasks into one raw task (reference nnunet/dataset_conversion/Task100_MultiTalent.py).

Tables: same names as the reference module (:35-207); the values are constant data stored in multitalent_tables.json (dumped by
tools/oracle_gen/dump_region_tables.py).  The trainers import them from here, so this module imports without a device.

Conversion (:210-401): every image of every source task is copied under `<task id>_<file name>`, every label file is mapped to
Task100's label values, and the six `cases_have_{labels,regions}_{tr,val,ts}` dictionaries plus `dataset.json` are written.
What the reference does per label file with `get_fdata()` (float64), `np.unique` and one masked assignment per label is one pass
of `mt_label_convert` over the volume in the type the file stores (`ops.label_convert`); the host builds the table
(`label_table`), plans the run (`plan_conversion`) and reads, compresses and writes the files.  There is no CPU fallback.
Differences from the reference, all recorded in DESIGN §6r: a `labels_out` above 255 is a ValueError (the reference wraps it
through uint8); the label file is stored as uint8 (the reference keeps the input header's dtype); an existing `labelsVal` target
is skipped like every other target unless `overwrite` is set (the reference converts it again on every run, with the same
result); `dataset.json` declares label 0 as `background` (the reference's does not, and its own integrity check rejects that)."""
import json
import numbers
import os
import pickle
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'multitalent_tables.json')) as _f:
    _T = json.load(_f)

# region name -> tuple of label values (47 regions; 3 are unions: 03_liver, 07_pancreas, 64_both_kidneys)
MultiTalent_regions = {k: tuple(v) for k, v in _T['MultiTalent_regions'].items()}
# region name -> network output channel (= enumeration order)
MultiTalent_region_output_idx_mapping = dict(_T['MultiTalent_region_output_idx_mapping'])
# source dataset -> regions that are annotated in it
MultiTalent_valid_regions = {k: tuple(v) for k, v in _T['MultiTalent_valid_regions'].items()}
MultiTalent_regions_class_order = {k: tuple(v) for k, v in _T['MultiTalent_regions_class_order'].items()}
MultiTalent_task_ids = _T['MultiTalent_task_ids']
MultiTalent_labels = _T['MultiTalent_labels']
MultiTalent_task_label_maps = _T['MultiTalent_task_label_maps']

LABEL_SLOTS, LABEL_UNLISTED = 1023, 0xffff           # MT_LABEL_SLOTS, MT_LABEL_UNLISTED of include/mtseg.h
SPLITS = ('Tr', 'Val', 'Ts')


def region_label_lut():
    """64-bit mask over label values for each output channel (consumed by mt_multitalent_loss_*)."""
    lut = [0] * len(MultiTalent_regions)
    for name, labels in MultiTalent_regions.items():
        m = 0
        for l in labels:
            assert 0 <= l < 64
            m |= (1 << l)
        lut[MultiTalent_region_output_idx_mapping[name]] = m
    return lut


def valid_mask(region_names):
    m = 0
    for r in region_names:
        m |= (1 << MultiTalent_region_output_idx_mapping[r])
    return m


def sanity_checks():
    """:210-215: the label values of a source task's valid regions are exactly the output labels of its label map."""
    for t, regions in MultiTalent_valid_regions.items():
        labels = sorted(set(i for r in regions for i in MultiTalent_regions[r]))
        assert len(labels) == len(MultiTalent_task_label_maps[t][1])
        assert all(i in MultiTalent_task_label_maps[t][1] for i in labels)


# ---- one label volume ------------------------------------------------------------------------------------------------------------
def _flat_labels(labels_in):
    flat = []
    for entry in labels_in:
        for label in (entry if hasattr(entry, '__len__') else (entry,)):
            if isinstance(label, bool) or not isinstance(label, numbers.Integral):
                raise ValueError("labels_in holds %r, which is no int" % (label,))
            flat.append(int(label))
    return flat


def label_table(labels_in, labels_out):
    """(labels_in, labels_out) of `copy_and_convert_segmentation` -> the uint16 table [LABEL_SLOTS] of `ops.label_convert`: the
    output 0..255 of every input label 0..1022, LABEL_UNLISTED where no pair lists it.  Entries of labels_in are ints or tuples of
    ints; the pairs are applied in order, so the LAST pair that lists a label wins: (1, 2, (3, 4), 3) -> (4, 5, 6, 7) gives
    1 -> 4, 2 -> 5, 4 -> 6, 3 -> 7.  An entry 0 is legal and never applies (a voxel has to exceed 1e-20 to be mapped).  An input
    label outside 0..1022 or an output outside 0..255 is a ValueError."""
    if len(labels_in) != len(labels_out):
        raise ValueError("labels_in has %d entries and labels_out %d" % (len(labels_in), len(labels_out)))
    table = np.full(LABEL_SLOTS, LABEL_UNLISTED, dtype=np.uint16)
    for entry, out in zip(labels_in, labels_out):
        if isinstance(out, bool) or not isinstance(out, numbers.Integral):
            raise ValueError("labels_out holds %r, which is no int" % (out,))
        if not 0 <= out <= 255:
            raise ValueError("labels_out holds %d: the converted volume is uint8 (0..255)" % out)
        for label in _flat_labels((entry,)):
            if not 0 <= label < LABEL_SLOTS:
                raise ValueError("labels_in holds %d: input labels run 0..%d" % (label, LABEL_SLOTS - 1))
            if label > 0:
                table[label] = out
    return table


_HOST_CASTS = {'int64': np.float64, 'uint64': np.float64, 'bool': np.uint8, 'float16': np.float32}


def _require_device():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("multitalent_amd: the label conversion of the dataset conversion runs on a HIP device only; there is no "
                           "CPU fallback")
    return torch


def copy_and_convert_segmentation(segmentation, labels_in, labels_out, sanity_check=True, in_file=None, keep_on_device=False):
    """:229-275.  segmentation: a numpy array (-> numpy uint8 array) or a device tensor (-> device uint8 tensor) in whatever type
    its file stores; int64 / uint64 are cast to float64 on the host, as `get_fdata` does.  A voxel not above 1e-20 (zero,
    negatives, NaN) becomes 0; a voxel that equals a listed label becomes that label's output (`label_table`); any other voxel
    becomes 0 and, with `sanity_check`, raises RuntimeError naming `in_file`, the smallest such value (the one the reference meets
    first) and the expected labels."""
    table = label_table(labels_in, labels_out)                   # ValueError before anything is uploaded
    torch = _require_device()
    from .. import ops
    as_numpy = not torch.is_tensor(segmentation)
    if as_numpy:
        a = np.asarray(segmentation)
        a = np.ascontiguousarray(a.astype(_HOST_CASTS[a.dtype.name]) if a.dtype.name in _HOST_CASTS else a)
        if a.dtype.name not in ops.LABEL_CONVERT_DTYPES:
            raise ValueError("copy_and_convert_segmentation: a %s volume is not supported" % a.dtype.name)
        if not a.dtype.isnative:
            a = a.astype(a.dtype.newbyteorder('='))
        seg = torch.from_numpy(a).cuda()
    else:
        seg = segmentation.contiguous()
        if seg.dtype in (torch.int64, torch.uint64):
            seg = seg.double()
    if seg.numel() == 0:
        out = torch.zeros(seg.shape, dtype=torch.uint8, device=seg.device)
        return out.cpu().numpy() if as_numpy and not keep_on_device else out
    out, count, smallest = ops.label_convert(seg, table)
    if sanity_check and count:
        raise RuntimeError("unexpected label in image %s: %r (%d voxels hold a value that is not among the expected labels %s)"
                           % (in_file, smallest, count, sorted(set(_flat_labels(labels_in)))))
    return out.cpu().numpy() if as_numpy and not keep_on_device else out


def copy_and_convert_segmentation_nifti(in_file, out_file, labels_in, labels_out, sanity_check=True):
    """:217-226 through utilities/nifti_io: the converted label file carries the input's geometry and is stored as uint8."""
    _write_label(out_file, _convert_label(_read_label(in_file), in_file, labels_in, labels_out, sanity_check, out_file.endswith('.nii.gz')))


def _read_label(in_file):
    from ..utilities.nifti_io import read_image
    return read_image(in_file)


def _convert_label(img, in_file, labels_in, labels_out, sanity_check=True, encode=False):
    """-> (converted uint8 volume, img).  encode (the target is a .nii.gz): the volume stays on the device and is gzip-encoded there;
    what comes back is the complete file as bytes, so that `_write_label` — a pool thread — only writes them."""
    if not encode or np.ndim(img.array) != 3:
        return copy_and_convert_segmentation(np.asarray(img.array), labels_in, labels_out, sanity_check, in_file), img
    from ..utilities.nifti_io import encode_label_map_device
    seg = copy_and_convert_segmentation(np.asarray(img.array), labels_in, labels_out, sanity_check, in_file, keep_on_device=True)
    return encode_label_map_device(seg, img.GetSpacing(), img.GetOrigin(), img.GetDirection()), img


def _write_label(out_file, converted):
    from ..utilities.nifti_io import write_image
    seg, img = converted
    if isinstance(seg, bytes):
        with open(out_file, 'wb') as f:
            f.write(seg)
        return
    write_image(seg, out_file, img.GetSpacing(), img.GetOrigin(), img.GetDirection())


# ---- the run ---------------------------------------------------------------------------------------------------------------------
def _nii(folder):
    return sorted(f for f in os.listdir(folder) if f.endswith('nii.gz') and os.path.isfile(os.path.join(folder, f)))


def plan_conversion(raw_data, tasks=None, task_name="Task100_MultiTalent", overwrite=False):
    """The host half of :279-401, no device.  raw_data: the `nnUNet_raw_data` folder; tasks: source task names (None: all 13).
    -> {'target_base', 'folders': the six target folders, 'copy': [(source image, target)], 'convert': [(source label file, target,
    labels_in, labels_out)], 'dictionaries': (cases_have_labels_tr, _val, _ts, cases_have_regions_tr, _val, _ts)}.
    A target is `<task id>_<file name>` with the id `t[4:7]`; imagesVal / labelsVal / imagesTs / labelsTs are taken where the source
    task has them.  A target that exists is left out of `copy` / `convert` unless `overwrite`; the dictionaries are keyed by the
    target label file name and hold every label file either way.  A missing source task is RuntimeError('missing task: ...')."""
    tasks = list(MultiTalent_task_label_maps.keys()) if tasks is None else list(tasks)
    target_base = os.path.join(raw_data, task_name)
    folders = {kind + s: os.path.join(target_base, kind + s) for s in SPLITS for kind in ('images', 'labels')}
    copy, convert = [], []
    labels = {s: {} for s in SPLITS}
    regions = {s: {} for s in SPLITS}
    for t in tasks:
        if t not in MultiTalent_task_label_maps:
            raise RuntimeError('unknown task: %s (the label maps know %s)' % (t, ', '.join(MultiTalent_task_label_maps)))
        task_id = t[4:7]
        source = os.path.join(raw_data, t)
        if not os.path.isdir(source):
            raise RuntimeError('missing task: %s' % t)
        labels_in, labels_out = (tuple(i) for i in MultiTalent_task_label_maps[t])
        for s in SPLITS:
            images, segs = os.path.join(source, 'images' + s), os.path.join(source, 'labels' + s)
            if s == 'Tr' or os.path.isdir(images):
                for i in _nii(images):
                    target = os.path.join(folders['images' + s], task_id + '_' + i)
                    if overwrite or not os.path.isfile(target):
                        copy.append((os.path.join(images, i), target))
            if s == 'Tr' or os.path.isdir(segs):
                for i in _nii(segs):
                    target = os.path.join(folders['labels' + s], task_id + '_' + i)
                    if overwrite or not os.path.isfile(target):
                        convert.append((os.path.join(segs, i), target, labels_in, labels_out))
                    labels[s][task_id + '_' + i] = labels_out
                    regions[s][task_id + '_' + i] = MultiTalent_valid_regions[t]
    return {'target_base': target_base, 'folders': folders, 'copy': copy, 'convert': convert,
            'dictionaries': tuple(labels[s] for s in SPLITS) + tuple(regions[s] for s in SPLITS)}


def convert_task100(task_name="Task100_MultiTalent", tasks=None, num_threads=8, overwrite=False):
    """:279-401.  A host pool of `num_threads` copies the images and reads and decompresses the label files, the label volumes go
    through the one device in sequence, and the same pool compresses and writes them behind it.  Writes
    `cases_have_regions_labels.pkl` (the six dictionaries) and `dataset.json` into the target task.  -> the plan it ran."""
    from .. import paths
    from .utils import generate_dataset_json
    plan = plan_conversion(paths.require(paths.nnUNet_raw_data), tasks, task_name, overwrite)
    _require_device()
    for folder in plan['folders'].values():
        os.makedirs(folder, exist_ok=True)
    workers = max(1, int(num_threads))
    jobs, to_copy = plan['convert'], list(plan['copy'])
    share = -(-len(to_copy) // max(1, len(jobs)))                     # image copies are dealt out between the label files, so that
    with ThreadPoolExecutor(max_workers=workers) as pool:             # the reads for the device never queue behind all of them
        reads, writes, copies = [], [], []
        for j in range(min(workers, len(jobs))):
            reads.append(pool.submit(_read_label, jobs[j][0]))
        for j, (src, dst, labels_in, labels_out) in enumerate(jobs):
            img = reads[j].result()
            reads[j] = None
            if j + workers < len(jobs):                               # bounds the volumes waiting in host memory
                reads.append(pool.submit(_read_label, jobs[j + workers][0]))
            copies += [pool.submit(shutil.copy, a, b) for a, b in to_copy[j * share:(j + 1) * share]]
            writes.append(pool.submit(_write_label, dst, _convert_label(img, src, labels_in, labels_out, encode=dst.endswith('.nii.gz'))))
            while len(writes) > 2 * workers:
                writes.pop(0).result()
        copies += [pool.submit(shutil.copy, a, b) for a, b in to_copy[len(jobs) * share:]]
        for f in writes + copies:
            f.result()
    labels = {0: 'background'}
    labels.update({int(k): v for k, v in MultiTalent_labels.items()})
    generate_dataset_json(os.path.join(plan['target_base'], 'dataset.json'), plan['folders']['imagesTr'], plan['folders']['imagesTs'],
                          ("CT",), labels, task_name)
    with open(os.path.join(plan['target_base'], 'cases_have_regions_labels.pkl'), 'wb') as f:
        pickle.dump(plan['dictionaries'], f)
    return plan


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Merge the MultiTalent source tasks of nnUNet_raw_data into Task100_MultiTalent.")
    ap.add_argument('-t', '--tasks', nargs='+', default=None, help="source task names; default: all 13")
    ap.add_argument('--task_name', default="Task100_MultiTalent")
    ap.add_argument('-tl', '--num_threads', type=int, default=8, help="host threads that read, compress and write")
    ap.add_argument('--overwrite', action='store_true', help="convert and copy again what is already there")
    a = ap.parse_args(argv)
    sanity_checks()
    plan = convert_task100(a.task_name, a.tasks, a.num_threads, a.overwrite)
    print("%s: %d images copied, %d label files converted" % (plan['target_base'], len(plan['copy']), len(plan['convert'])))


if __name__ == '__main__':
    main(sys.argv[1:])
