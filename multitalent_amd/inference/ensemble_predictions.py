"""`nnUNet_ensemble` on the device (reference nnunet/inference/ensemble_predictions.py:26-124): the same entry points (`merge_files`,
`merge`, `main` with `-f -o -t -pp --npz`), the same folder scan and assertions, the same files (`<out>/<case>.nii.gz`, with
`--npz` the float16 mean as `softmax` in `<case>.npz` and the LIST of member properties in `<case>.pkl`, with `-pp` the raw masks
under `not_postprocessed/`, the post-processed ones in `<out>` and a copy of the json).

What is different underneath: the reference's `np.vstack` -> `np.mean` -> argmax / region thresholds -> insertion into the uncropped
volume (four host passes over K*C*V elements) is ONE kernel, `mt_ensemble_classify`, which reproduces numpy's float16 mean bit for
bit and decides the label on it.  The members are the stored probabilities at the original grid, so nothing is resampled: a member
whose shape is not `size_after_cropping` (neither exporter writes one) is refused.  `threads` is accepted and ignored; the compressed
members of the next case are read and inflated on the device from one host thread while the current case is merged."""
import argparse
import os
import pickle
import shutil
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import _lib

MAX_MEMBERS = 16                      # MT_ENSEMBLE_MAX_MEMBERS of include/mtseg.h
VEC = 8                               # float16 elements of one 16-byte access


def padded_stride(V):
    """Channel stride of the device layout: the next multiple of 8 elements, so that every channel starts on 16 bytes."""
    return (int(V) + VEC - 1) // VEC * VEC


def ensemble_classify(members, C, shape, chan_stride, out, offset, class_order=None, mean=None, mean_stride=0):
    """One launch of `mt_ensemble_classify`.  members: K float16 device tensors holding [C][chan_stride] elements each (any
    2-byte aligned view); shape: the box (D, H, W); out: uint8 device tensor [FD, FH, FW], written at `offset`; class_order: None
    (argmax) or an int32 device tensor [C]; mean: None or a float16 device tensor for [C][mean_stride]."""
    import ctypes
    import torch
    K = len(members)
    if not 1 <= K <= MAX_MEMBERS:
        raise ValueError("an ensemble takes 1 .. %d members, got %d" % (MAX_MEMBERS, K))
    D, H, W = (int(i) for i in shape)
    need = (C - 1) * int(chan_stride) + D * H * W
    for m in members:
        assert m.is_cuda and m.dtype == torch.float16 and m.numel() >= need, "members: float16 device tensors of [C][chan_stride]"
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 3 and out.is_contiguous()
    assert mean is None or (mean.is_cuda and mean.dtype == torch.float16 and mean.numel() >= (C - 1) * int(mean_stride) + D * H * W)
    assert class_order is None or (class_order.is_cuda and class_order.dtype == torch.int32 and class_order.numel() == C)
    ptrs = (ctypes.c_void_p * K)(*[m.data_ptr() for m in members])
    lib = _lib.load()
    _lib.check(lib.mt_ensemble_classify(ptrs, K, int(C), D, H, W, int(chan_stride),
                                        class_order.data_ptr() if class_order is not None else None,
                                        1 if class_order is not None else 0, out.data_ptr(), int(out.shape[0]), int(out.shape[1]),
                                        int(out.shape[2]), int(offset[0]), int(offset[1]), int(offset[2]),
                                        mean.data_ptr() if mean is not None else None, int(mean_stride),
                                        torch.cuda.current_stream(out.device).cuda_stream), 'ensemble_classify')
    return out


def upload_member(arr, device):
    """float16 [C, X, Y, Z], on the host or (read by `load_npz_device`) on the device -> [C, padded_stride(V)] on the device (the
    pad is never read as a voxel)."""
    import torch
    C = int(arr.shape[0])
    V = int(np.prod(arr.shape[1:]))
    buf = torch.empty((C, padded_stride(V)), dtype=torch.float16, device=device)
    if torch.is_tensor(arr):
        buf[:, :V].copy_(arr.reshape(C, V))
    else:
        buf[:, :V].copy_(torch.from_numpy(np.ascontiguousarray(arr).reshape(C, V)))
    return buf


def merge_on_device(arrays, properties, regions_class_order=None, want_mean=False, device=None, keep_on_device=False,
                    mean_on_device=False):
    """K float16 arrays [C, X, Y, Z] (X, Y, Z = size_after_cropping of `properties`) -> (uint8 label volume of
    `original_size_of_raw_data` as numpy — as a device tensor with `keep_on_device`, for the device file writer —, float16 mean
    [C, X, Y, Z] as numpy or None — with `mean_on_device` as a device tensor, a view of the padded rows the kernel wrote, for
    utilities.npz_io.save_npz_device)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("multitalent_amd: ensembling runs on a HIP device only; there is no CPU fallback")
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    C = int(arrays[0].shape[0])
    shape = tuple(int(i) for i in arrays[0].shape[1:])
    V = int(np.prod(shape))
    bbox = properties.get('crop_bbox')
    if bbox is not None:
        full = [int(i) for i in properties.get('original_size_of_raw_data')]
        lo = [int(bbox[c][0]) for c in range(3)]
        if any(lo[c] + shape[c] > full[c] for c in range(3)):
            raise ValueError("crop_bbox + size_after_cropping exceeds original_size_of_raw_data")     # the reference fails here too
    else:
        full, lo = list(shape), [0, 0, 0]
    cs = padded_stride(V)
    members = [upload_member(a, device) for a in arrays]
    out = torch.zeros(full, dtype=torch.uint8, device=device)
    order_t = None
    if regions_class_order is not None:
        order_t = torch.tensor([int(np.asarray(c).reshape(-1)[0]) for c in regions_class_order], dtype=torch.int32, device=device)
        assert order_t.numel() == C, "one class per channel expected in regions_class_order"
    mean = torch.empty((C, cs), dtype=torch.float16, device=device) if want_mean else None
    ensemble_classify(members, C, shape, cs, out, lo, order_t, mean, cs)
    if want_mean and mean_on_device:
        return (out if keep_on_device else out.cpu().numpy()), mean[:, :V].unflatten(1, shape)
    mean_np = mean[:, :V].cpu().numpy().reshape((C,) + shape) if want_mean else None
    return (out if keep_on_device else out.cpu().numpy()), mean_np


def _load_pickle(f):
    with open(f, 'rb') as fh:
        return pickle.load(fh)


def _read_member(f, device=None):
    """the stored probabilities of one member: inflated on `device` (utilities.npz_io.load_npz_device; a file of another writer
    falls back to np.load there) when there is one, so that the rejections below still work without.  device None: the calling
    thread's current device — a pool thread passes the one its caller selected."""
    import torch
    if torch.cuda.is_available():
        from ..utilities.npz_io import load_npz_device
        return load_npz_device(f, 'softmax', torch.device('cuda', torch.cuda.current_device()) if device is None else device)
    return np.load(f)['softmax']


def _load_case(files, properties_files, device=None):
    """One case: the K members (device tensors when there is a device) and their properties, with every rejection."""
    if len(files) > MAX_MEMBERS:
        raise ValueError("an ensemble takes at most %d members, got %d: %s" % (MAX_MEMBERS, len(files), str(files)))
    props = [_load_pickle(f) for f in properties_files]
    after = tuple(int(i) for i in props[0]['size_after_cropping'])
    arrays = []
    for f in files:
        a = _read_member(f, device)
        if str(a.dtype).replace('torch.', '') != 'float16':
            raise TypeError("%s: softmax is %s, the exporters store float16" % (f, a.dtype))
        if tuple(a.shape[1:]) != after or (arrays and a.shape != arrays[0].shape):
            raise NotImplementedError("%s: softmax of shape %s, size_after_cropping is %s: stored probabilities are at the original "
                                      "grid, nothing is resampled here" % (f, tuple(a.shape), after))
        arrays.append(a)
    if arrays[0].shape[0] > 255:
        raise ValueError("%s: %d channels, the label volume is uint8" % (files[0], arrays[0].shape[0]))
    orders = [p.get('regions_class_order') for p in props]
    if any(o is not None for o in orders):            # region models: every member must paint in the same order (:33-45)
        assert all(o == orders[0] for o in orders[1:]), \
            'If merging files with regions_class_order, the regions_class_orders of all ' \
            'files must be the same. regions_class_order: %s, \n files: %s' % (str(orders), str(files))
    return arrays, props, orders[0]


def merge_files(files, properties_files, out_file, override, store_npz, _loaded=None):
    """reference :26-53.  `_loaded`: the result of `_load_case` when the caller has read the members already."""
    from ..utilities.nifti_io import write_image
    if override or not os.path.isfile(out_file):
        arrays, props, regions_class_order = _loaded if _loaded is not None else _load_case(files, properties_files)
        seg, mean = merge_on_device(arrays, props[0], regions_class_order, want_mean=store_npz, keep_on_device=out_file.endswith('.nii.gz'),
                                    mean_on_device=True)
        write_image(seg, out_file, props[0]['itk_spacing'], props[0]['itk_origin'], props[0]['itk_direction'])
        if store_npz:
            from ..utilities.npz_io import save_npz_device
            save_npz_device(out_file[:-7] + ".npz", softmax=mean)
            with open(out_file[:-7] + ".pkl", 'wb') as f:
                pickle.dump(props, f)


def _subfiles(folder, suffix):
    return sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(suffix))


def merge(folders, output_folder, threads, override=True, postprocessing_file=None, store_npz=False):
    """reference :56-95."""
    from ..postprocessing.connected_components import apply_postprocessing_to_folder, load_postprocessing
    os.makedirs(output_folder, exist_ok=True)
    if postprocessing_file is not None:
        output_folder_orig = output_folder
        output_folder = os.path.join(output_folder, 'not_postprocessed')
        os.makedirs(output_folder, exist_ok=True)
    else:
        output_folder_orig = None

    patient_ids = [i[:-4] for f in folders for i in _subfiles(f, ".npz")]
    patient_ids = np.unique(patient_ids)
    for f in folders:
        assert all([os.path.isfile(os.path.join(f, i + ".npz")) for i in patient_ids]), "Not all patient npz are available in " \
                                                                                         "all folders"
        assert all([os.path.isfile(os.path.join(f, i + ".pkl")) for i in patient_ids]), "Not all patient pkl are available in " \
                                                                                         "all folders"
    jobs = []
    for p in patient_ids:
        out_file = os.path.join(output_folder, p + ".nii.gz")
        if override or not os.path.isfile(out_file):
            jobs.append(([os.path.join(f, p + ".npz") for f in folders], [os.path.join(f, p + ".pkl") for f in folders], out_file))
    # the members of the next case are read and decompressed while the current one is on the device
    import torch
    device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None     # (per thread: handed to the pool)
    with ThreadPoolExecutor(1) as ex:
        nxt = ex.submit(_load_case, jobs[0][0], jobs[0][1], device) if jobs else None
        for n, (files, property_files, out_file) in enumerate(jobs):
            loaded = nxt.result()
            nxt = ex.submit(_load_case, jobs[n + 1][0], jobs[n + 1][1], device) if n + 1 < len(jobs) else None
            merge_files(files, property_files, out_file, True, store_npz, _loaded=loaded)

    if postprocessing_file is not None:
        for_which_classes, min_valid_obj_size = load_postprocessing(postprocessing_file)
        print('Postprocessing...')
        apply_postprocessing_to_folder(output_folder, output_folder_orig, for_which_classes, min_valid_obj_size, threads)
        shutil.copy(postprocessing_file, output_folder_orig)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Merge the stored probabilities (.npz + .pkl, written with --save_npz) of several "
                                                 "prediction folders into one segmentation per case.")
    parser.add_argument('-f', '--folders', nargs='+', required=True, help="the member folders (2 .. 16)")
    parser.add_argument('-o', '--output_folder', required=True, type=str)
    parser.add_argument('-t', '--threads', required=False, default=2, type=int, help="accepted and ignored: the merge runs on the device")
    parser.add_argument('-pp', '--postprocessing_file', required=False, type=str, default=None,
                        help="postprocessing.json to apply to the merged masks; without it there is no post-processing")
    parser.add_argument('--npz', action="store_true", required=False, help="also store the mean probabilities (.npz) and the properties (.pkl)")
    args = parser.parse_args(argv)
    merge(args.folders, args.output_folder, args.threads, override=True, postprocessing_file=args.postprocessing_file,
          store_npz=args.npz)


if __name__ == "__main__":
    main()
