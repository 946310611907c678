"""Connected-component postprocessing (reference postprocessing/connected_components.py): "keep only the largest connected
component" per class entry, and the per-fold search `determine_postprocessing` that `nnUNetTrainer.validate` ends in.

The labelling is the device's (`mt_cc_label3d` / `mt_cc_remove`: 6-connected union-find with exact sizes, include/mtseg.h);
everything around it — file I/O, the Dice bookkeeping through `evaluation.evaluator.aggregate_scores`, the decisions and
`postprocessing.json` — is host code restating the reference line by line.  There is no CPU labelling: without a HIP device
the functions raise.  The reference's process pool is not used: cases run one after another on the device (`processes` /
`num_processes` are accepted and ignored)."""
import ast
import json
import os
import shutil
from copy import deepcopy

import numpy as np
import torch

from .. import ops
from ..evaluation.evaluator import aggregate_scores
from ..utilities.nifti_io import Image, read_image, read_image_device, write_image

default_num_threads = 8


def _no_device():
    raise RuntimeError("multitalent_amd: connected-component post-processing runs on a HIP device only; there is no CPU fallback")


def _to_device_uint8(image):
    """-> (contiguous uint8 device tensor, device); values outside 0..255 are rejected before anything is launched."""
    if torch.is_tensor(image):
        if not image.is_cuda:
            _no_device()
        if image.dtype == torch.uint8:
            return image.contiguous(), image.device
        if image.dtype.is_floating_point or image.dtype.is_complex:
            raise ValueError("connected components: an integer label volume is expected, got %s" % image.dtype)
        if image.numel() and (int(image.min()) < 0 or int(image.max()) > 255):
            raise ValueError("connected components: label values must lie in 0..255")
        return image.to(torch.uint8).contiguous(), image.device
    if not torch.cuda.is_available():
        _no_device()
    a = np.asarray(image)
    if a.dtype != np.uint8:
        if a.dtype.kind not in 'biu':
            raise ValueError("connected components: an integer label volume is expected, got %s" % a.dtype)
        if a.size and (int(a.min()) < 0 or int(a.max()) > 255):
            raise ValueError("connected components: label values must lie in 0..255")
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev), dev


def remove_all_but_the_largest_connected_component(image, for_which_classes, volume_per_voxel, minimum_valid_object_size=None):
    """connected_components.py:48-101.  image: numpy array (modified in place, as in the reference) or HIP device tensor
    [D, H, W] of integer labels in 0..255.  for_which_classes: None (every label > 0 present), or a list of ints and
    tuples (a tuple is one joint mask); entries are processed in order, each on the image as the previous one left it.
    Returns (image, largest_removed, kept_size): dicts keyed by the entries (ints, tuples), values None or fp64 sizes
    (voxel count * volume_per_voxel)."""
    ops.cc_check_shape(np.shape(image) if not torch.is_tensor(image) else image.shape)
    seg, dev = _to_device_uint8(image)
    if for_which_classes is None:
        present = torch.unique(seg).cpu().numpy()
        for_which_classes = [int(i) for i in present[present > 0]]
    assert 0 not in for_which_classes, "cannot remove background"
    vpv = float(volume_per_voxel)
    largest_removed, kept_size = {}, {}
    if len(for_which_classes) == 0:
        return image, largest_removed, kept_size
    with torch.cuda.device(dev):
        labels = torch.empty(seg.shape, dtype=torch.int32, device=dev)
        sizes = torch.empty(seg.shape, dtype=torch.int32, device=dev)
        stats = torch.empty(3, dtype=torch.int32, device=dev)      # components, largest count, largest removed count
        for c in for_which_classes:
            if isinstance(c, (list, tuple)):
                c = tuple(c)
                members = c
            else:
                c = int(c)
                members = (c,)
            member = np.zeros(256, dtype=bool)
            for m in members:
                if 0 <= int(m) <= 255:
                    member[int(m)] = True
            ops.cc_label3d(seg, member, labels, sizes, stats[:2])
            min_size = None
            if minimum_valid_object_size is not None:
                if c in minimum_valid_object_size:
                    min_size = float(minimum_valid_object_size[c])
                elif int(stats[0]) > 1:
                    # the reference looks the entry up only when there is a component besides the largest to judge
                    raise KeyError(c)
            ops.cc_remove(seg, labels, sizes, stats[:2], vpv, None if min_size is None else float(min_size), stats[2:])
            n, mx, rem = (int(i) for i in stats.cpu())
            largest_removed[c] = float(np.float64(rem) * np.float64(vpv)) if rem > 0 else None
            kept_size[c] = float(np.float64(mx) * np.float64(vpv)) if n > 0 else None
    if torch.is_tensor(image):
        if seg.data_ptr() != image.data_ptr():
            image.copy_(seg)
    else:
        image[...] = seg.cpu().numpy()
    return image, largest_removed, kept_size


def load_remove_save(input_file, output_file, for_which_classes, minimum_valid_object_size=None):
    """connected_components.py:30-45: the file's geometry is kept, volume_per_voxel = prod(spacing) in fp64."""
    if input_file.endswith('.nii.gz') and output_file.endswith('.nii.gz') and torch.cuda.is_available():
        # inflated on the device (utilities.nifti_io.read_image_device); a uint8 label map never visits the host
        vox, spacing, origin, direction = read_image_device(input_file, torch.device('cuda', torch.cuda.current_device()))
        img = Image(vox if vox.dtype == torch.uint8 else vox.cpu().numpy(), spacing, origin, direction)
    else:
        img = read_image(input_file)
    volume_per_voxel = float(np.prod(img.spacing, dtype=np.float64))
    if torch.is_tensor(img.array):
        ops.cc_check_shape(tuple(img.array.shape))
        img_npy = img.array
    else:
        img_npy = np.asarray(img.array)
    if not torch.is_tensor(img_npy) and img_npy.dtype == np.uint8 and img_npy.ndim == 3 and output_file.endswith('.nii.gz'):
        # the label map stays on the device after the removal and is written from there (utilities.nifti_io.write_label_map_device)
        ops.cc_check_shape(img_npy.shape)
        img_npy = _to_device_uint8(img_npy)[0]
    image, largest_removed, kept_size = remove_all_but_the_largest_connected_component(img_npy, for_which_classes, volume_per_voxel,
                                                                                       minimum_valid_object_size)
    write_image(image, output_file, img.spacing, img.origin, img.direction)
    return largest_removed, kept_size


def _load_json(f):
    with open(f) as fh:
        return json.load(fh)


def _save_json(obj, f):
    with open(f, 'w') as fh:
        json.dump(obj, fh, sort_keys=True, indent=4)


def _subfiles(folder, suffix):
    return sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(suffix))


def load_postprocessing(json_file):
    """connected_components.py:104-116 -> (for_which_classes, min_valid_object_sizes)."""
    a = _load_json(json_file)
    if 'min_valid_object_sizes' in a.keys():
        min_valid_object_sizes = ast.literal_eval(a['min_valid_object_sizes'])
    else:
        min_valid_object_sizes = None
    return a['for_which_classes'], min_valid_object_sizes


def _aggregate_sizes(results):
    """max of largest_removed / min of kept_size over the cases (connected_components.py:183-199, 282-298)."""
    max_size_removed, min_size_kept = {}, {}
    for mx_rem, min_kept in results:
        for k in mx_rem:
            if mx_rem[k] is not None:
                max_size_removed[k] = mx_rem[k] if max_size_removed.get(k) is None else max(max_size_removed[k], mx_rem[k])
        for k in min_kept:
            if min_kept[k] is not None:
                min_size_kept[k] = min_kept[k] if min_size_kept.get(k) is None else min(min_size_kept[k], min_kept[k])
    return max_size_removed, min_size_kept


def determine_postprocessing(base, gt_labels_folder, raw_subfolder_name="validation_raw", temp_folder="temp",
                             final_subf_name="validation_final", processes=default_num_threads, dice_threshold=0, debug=False,
                             advanced_postprocessing=False, pp_filename="postprocessing.json"):
    """connected_components.py:119-397: does removing all but the largest connected component improve Dice, first for all
    foreground classes as one region, then for each class on its own?  Writes `<base>/<pp_filename>` and the post-processed
    predictions with their summary.json to `<base>/<final_subf_name>`; the temp folders are deleted unless `debug`."""
    classes = [int(i) for i in _load_json(os.path.join(base, raw_subfolder_name, "summary.json"))['results']['mean'].keys()
               if int(i) != 0]
    folder_all_classes_as_fg = os.path.join(base, temp_folder + "_allClasses")
    folder_per_class = os.path.join(base, temp_folder + "_perClass")
    if os.path.isdir(folder_all_classes_as_fg):
        shutil.rmtree(folder_all_classes_as_fg)
    if os.path.isdir(folder_per_class):
        shutil.rmtree(folder_per_class)
    assert os.path.isfile(os.path.join(base, raw_subfolder_name, "summary.json")), \
        "join(base, raw_subfolder_name) does not contain a summary.json"
    fnames = _subfiles(os.path.join(base, raw_subfolder_name), ".nii.gz")
    os.makedirs(folder_all_classes_as_fg, exist_ok=True)
    os.makedirs(folder_per_class, exist_ok=True)
    os.makedirs(os.path.join(base, final_subf_name), exist_ok=True)

    pp_results = {'dc_per_class_raw': {}, 'dc_per_class_pp_all': {}, 'dc_per_class_pp_per_class': {}, 'for_which_classes': [],
                  'min_valid_object_sizes': {}}
    validation_result_raw = _load_json(os.path.join(base, raw_subfolder_name, "summary.json"))['results']
    pp_results['num_samples'] = len(validation_result_raw['all'])
    validation_result_raw = validation_result_raw['mean']

    if advanced_postprocessing:
        results = [load_remove_save(os.path.join(base, raw_subfolder_name, f), os.path.join(folder_all_classes_as_fg, f),
                                    (classes,)) for f in fnames]
        _, min_size_kept = _aggregate_sizes(results)
        print("foreground vs background, smallest valid object size was", min_size_kept[tuple(classes)])
        print("removing only objects smaller than that...")
    else:
        min_size_kept = None

    # all foreground classes as one region
    pred_gt_tuples = []
    for f in fnames:
        output_file = os.path.join(folder_all_classes_as_fg, f)
        load_remove_save(os.path.join(base, raw_subfolder_name, f), output_file, (classes,), min_size_kept)
        pred_gt_tuples.append([output_file, os.path.join(gt_labels_folder, f)])
    aggregate_scores(pred_gt_tuples, labels=classes, json_output_file=os.path.join(folder_all_classes_as_fg, "summary.json"),
                     json_author="Fabian", num_threads=processes)
    validation_result_PP_test = _load_json(os.path.join(folder_all_classes_as_fg, "summary.json"))['results']['mean']
    for c in classes:
        pp_results['dc_per_class_raw'][str(c)] = validation_result_raw[str(c)]['Dice']
        pp_results['dc_per_class_pp_all'][str(c)] = validation_result_PP_test[str(c)]['Dice']

    # accepted when at least one class improves and none gets worse (:236-257)
    do_fg_cc = False
    comp = [pp_results['dc_per_class_pp_all'][str(cl)] > (pp_results['dc_per_class_raw'][str(cl)] + dice_threshold) for cl in classes]
    before = np.mean([pp_results['dc_per_class_raw'][str(cl)] for cl in classes])
    after = np.mean([pp_results['dc_per_class_pp_all'][str(cl)] for cl in classes])
    print("Foreground vs background")
    print("before:", before)
    print("after: ", after)
    if any(comp):
        any_worse = any(pp_results['dc_per_class_pp_all'][str(cl)] < pp_results['dc_per_class_raw'][str(cl)] for cl in classes)
        if not any_worse:
            pp_results['for_which_classes'].append(classes)
            if min_size_kept is not None:
                pp_results['min_valid_object_sizes'].update(deepcopy(min_size_kept))
            do_fg_cc = True
            print("Removing all but the largest foreground region improved results!")
            print('for_which_classes', classes)
            print('min_valid_object_sizes', min_size_kept)

    if len(classes) > 1:
        source = folder_all_classes_as_fg if do_fg_cc else os.path.join(base, raw_subfolder_name)
        if advanced_postprocessing:
            results = [load_remove_save(os.path.join(source, f), os.path.join(folder_per_class, f), classes) for f in fnames]
            _, min_size_kept = _aggregate_sizes(results)
            print("classes treated separately, smallest valid object sizes are")
            print(min_size_kept)
            print("removing only objects smaller than that")
        else:
            min_size_kept = None
        pred_gt_tuples = []
        for f in fnames:
            output_file = os.path.join(folder_per_class, f)
            load_remove_save(os.path.join(source, f), output_file, classes, min_size_kept)
            pred_gt_tuples.append([output_file, os.path.join(gt_labels_folder, f)])
        aggregate_scores(pred_gt_tuples, labels=classes, json_output_file=os.path.join(folder_per_class, "summary.json"),
                         json_author="Fabian", num_threads=processes)
        old_res = deepcopy(validation_result_PP_test) if do_fg_cc else validation_result_raw
        validation_result_PP_test = _load_json(os.path.join(folder_per_class, "summary.json"))['results']['mean']
        for c in classes:
            dc_raw = old_res[str(c)]['Dice']
            dc_pp = validation_result_PP_test[str(c)]['Dice']
            pp_results['dc_per_class_pp_per_class'][str(c)] = dc_pp
            print(c)
            print("before:", dc_raw)
            print("after: ", dc_pp)
            if dc_pp > (dc_raw + dice_threshold):
                pp_results['for_which_classes'].append(int(c))
                if min_size_kept is not None:
                    pp_results['min_valid_object_sizes'].update({c: min_size_kept[c]})
                print("Removing all but the largest region for class %d improved results!" % c)
                print('min_valid_object_sizes', min_size_kept)
    else:
        print("Only one class present, no need to do each class separately as this is covered in fg vs bg")

    if not advanced_postprocessing:
        pp_results['min_valid_object_sizes'] = None
    print("done")
    print("for which classes:")
    print(pp_results['for_which_classes'])
    print("min_object_sizes")
    print(pp_results['min_valid_object_sizes'])
    pp_results['validation_raw'] = raw_subfolder_name
    pp_results['validation_final'] = final_subf_name

    # apply the decisions to the raw predictions
    pred_gt_tuples = []
    for f in fnames:
        output_file = os.path.join(base, final_subf_name, f)
        load_remove_save(os.path.join(base, raw_subfolder_name, f), output_file, pp_results['for_which_classes'],
                         pp_results['min_valid_object_sizes'])
        pred_gt_tuples.append([output_file, os.path.join(gt_labels_folder, f)])
    aggregate_scores(pred_gt_tuples, labels=classes, json_output_file=os.path.join(base, final_subf_name, "summary.json"),
                     json_author="Fabian", num_threads=processes)
    pp_results['min_valid_object_sizes'] = str(pp_results['min_valid_object_sizes'])
    _save_json(pp_results, os.path.join(base, pp_filename))
    if not debug:
        shutil.rmtree(folder_per_class)
        shutil.rmtree(folder_all_classes_as_fg)
    print("done")


def apply_postprocessing_to_folder(input_folder, output_folder, for_which_classes, min_valid_object_size=None, num_processes=8):
    """connected_components.py:400-421: load_remove_save for every .nii.gz of a folder."""
    os.makedirs(output_folder, exist_ok=True)
    for f in _subfiles(input_folder, ".nii.gz"):
        load_remove_save(os.path.join(input_folder, f), os.path.join(output_folder, f), for_which_classes, min_valid_object_size)
