"""One case end to end on the device (SURVEY §3.2 call stack, predict_MultiTalent.py:222-266 + preprocessing.py:226-311 +
segmentation_export.py:27-160): cropped CT -> resample to the plan spacing + clip/z-score -> sliding window (Gaussian weighting,
optional mirroring) -> probabilities resampled to the original grid, thresholded per region and re-inserted into the uncropped
volume.  The volume never leaves HBM between the stages.  The crop to the non-zero region in front of this chain is on the
device too (`preprocessing.device_cropping.crop_to_nonzero`, which `GenericPreprocessor.preprocess_test_case` uses); reading the
image and writing the NIfTI stay with the caller (SimpleITK).

`predict_cases` / `predict_from_folder` are the stock `nnUNet_predict` drivers (reference nnunet/inference/predict.py:131-291,
603-692) for an ordinary softmax model, such as one fine-tuned from the MultiTalent weights: the device flow of
`predict_MultiTalent.predict_cases` (preprocess on the device, ensemble the folds in HBM, transpose back) with the stock tail: one
`<out>/<case>.nii.gz` per case, `<case>.npz` / `.pkl` with `save_npz`, and the model folder's `postprocessing.json` copied and
applied.  `num_threads_preprocessing` / `num_threads_nifti_save` are accepted and ignored."""
import os
import pickle
import shutil

import numpy as np

from ..preprocessing.device_preprocessing import resample_and_normalize_ct
from .segmentation_export import resample_and_classify
from .sliding_window import predict_3D
from .predict_MultiTalent import _export_params, check_input_folder_and_return_caseIDs  # noqa: F401 (re-exported)


def predict_case_on_device(network, cropped_data, properties, target_spacing, intensityproperties, patch_size,
                           regions_class_order=None, do_mirroring=True, mirror_axes=(0, 1, 2), step_size=0.5,
                           transpose_forward=(0, 1, 2), force_separate_z=None, tile_shard=None, verbose=False,
                           transpose_backward=None, mixed_precision=True):
    """The chain: `device_cropping.crop_to_nonzero` (the caller's, see above) -> `resample_and_normalize_ct` -> `predict_3D` ->
    `resample_and_classify`.
    cropped_data: [C, X, Y, Z] (numpy or device tensor) already transposed by `transpose_forward`; properties: the case's
    dict (`original_spacing`, `size_after_cropping`, `original_size_of_raw_data`, `crop_bbox`).  Returns the uint8 label volume
    (device tensor, shape `original_size_of_raw_data`) and the properties with the resampling entries filled in.
    mixed_precision: the reference's predict default (predict_MultiTalent.py `--disable_mixed_precision` turns it off); False = the fp32 parity path."""
    spacing = np.array(properties['original_spacing'])[list(transpose_forward)]
    x = resample_and_normalize_ct(cropped_data, spacing, target_spacing, intensityproperties, force_separate_z)
    properties = dict(properties)
    properties['size_after_resampling'] = tuple(int(i) for i in x.shape[1:])
    properties['spacing_after_resampling'] = np.array(target_spacing)
    if tile_shard is not None and tile_shard[1] > 1:
        # tiles sharded over the ranks; the export below needs whole x-columns of the probabilities, so the slabs are gathered
        # (every rank then holds the full result)
        _, probs = predict_3D(network, x, do_mirroring, mirror_axes, True, step_size, patch_size, regions_class_order, True,
                              'constant', None, True, verbose, mixed_precision, tile_shard=tile_shard, return_device_tensors='full')
    else:
        _, probs = predict_3D(network, x, do_mirroring, mirror_axes, True, step_size, patch_size, regions_class_order, True,
                              'constant', None, True, verbose, mixed_precision, return_device_tensors=True)
    # the reference transposes the probabilities back before the export matches them to size_after_cropping / crop_bbox
    # (predict_MultiTalent.py:238-240: softmax.transpose([0] + [i + 1 for i in transpose_backward]))
    if transpose_backward is None:
        transpose_backward = [int(i) for i in np.argsort(list(transpose_forward))]
    if list(transpose_backward) != [0, 1, 2]:
        probs = probs.permute(0, *[int(i) + 1 for i in transpose_backward]).contiguous()
    seg = resample_and_classify(probs, properties, regions_class_order, 1, force_separate_z, 0)
    return seg, properties


def predict_cases(model, list_of_lists, output_filenames, folds, save_npz, num_threads_preprocessing, num_threads_nifti_save,
                  segs_from_prev_stage=None, do_tta=True, mixed_precision=True, overwrite_existing=False, all_in_gpu=False,
                  step_size=0.5, checkpoint_name="model_final_checkpoint", segmentation_export_kwargs=None,
                  disable_postprocessing=False):
    """reference :131-291.  model: folder with the fold_x subfolders; list_of_lists: [[case0_0000.nii.gz, ...], ...];
    output_filenames: [case0.nii.gz, ...]."""
    from ..postprocessing.connected_components import load_postprocessing, load_remove_save
    from ..training.model_restore import load_model_and_checkpoint_files
    from .segmentation_export import save_segmentation_nifti_from_softmax
    assert len(list_of_lists) == len(output_filenames)
    if segs_from_prev_stage is not None:
        raise NotImplementedError("cascade inputs (segs_from_prev_stage) are not on this path")
    cleaned = []
    for o in output_filenames:
        dr, f = os.path.split(o)
        if len(dr) > 0:
            os.makedirs(dr, exist_ok=True)
        if not f.endswith(".nii.gz"):
            f = os.path.splitext(f)[0] + ".nii.gz"
        cleaned.append(os.path.join(dr, f))
    if not overwrite_existing:
        print("number of cases:", len(list_of_lists))
        todo = [i for i, j in enumerate(cleaned) if (not os.path.isfile(j)) or (save_npz and not os.path.isfile(j[:-7] + '.npz'))]
        cleaned = [cleaned[i] for i in todo]
        list_of_lists = [list_of_lists[i] for i in todo]
        print("number of cases that still need to be predicted:", len(cleaned))
    print("loading parameters for folds,", folds)
    trainer, params = load_model_and_checkpoint_files(model, folds, mixed_precision=mixed_precision, checkpoint_name=checkpoint_name)
    force_separate_z, order, order_z = _export_params(trainer, segmentation_export_kwargs)
    region_class_order = trainer.regions_class_order if hasattr(trainer, 'regions_class_order') else None
    print("starting prediction...")
    for input_files, output_filename in zip(list_of_lists, cleaned):
        try:
            d, _, dct = trainer.preprocess_patient(input_files, return_device=True)
        except KeyboardInterrupt:
            raise
        except Exception as e:                        # the reference's workers skip a broken case and report it (:79-83)
            print("error in", input_files)
            print(e)
            continue
        print("predicting", output_filename)
        probs = None
        for p in params:
            trainer.load_checkpoint_ram(p, False)
            cur = trainer.predict_preprocessed_data_return_seg_and_softmax(
                d, do_mirroring=do_tta, mirror_axes=trainer.data_aug_params['mirror_axes'], use_sliding_window=True,
                step_size=step_size, use_gaussian=True, all_in_gpu=all_in_gpu, mixed_precision=mixed_precision,
                return_device_tensors=True)[1]
            # `cur` aliases the network's sliding-window cache: an ensemble accumulates into its own copy
            probs = (cur.clone() if len(params) > 1 else cur) if probs is None else probs.add_(cur)
        if len(params) > 1:
            probs /= len(params)
        if trainer.plans.get('transpose_forward') is not None:
            tb = trainer.plans.get('transpose_backward')
            if list(tb) != [0, 1, 2]:
                probs = probs.permute(0, *[int(i) + 1 for i in tb]).contiguous()
        save_segmentation_nifti_from_softmax(probs, output_filename, dct, order, region_class_order, None, None,
                                             output_filename[:-7] + ".npz" if save_npz else None, None, force_separate_z, order_z)
    print("inference done.")
    if not disable_postprocessing:
        pp_file = os.path.join(model, "postprocessing.json")
        if os.path.isfile(pp_file):
            print("postprocessing...")
            shutil.copy(pp_file, os.path.abspath(os.path.dirname(output_filenames[0])))
            for_which_classes, min_valid_obj_size = load_postprocessing(pp_file)
            for f in output_filenames:
                load_remove_save(f, f, for_which_classes, min_valid_obj_size)
        else:
            print("WARNING! Cannot run postprocessing because the postprocessing file is missing. Make sure to run "
                  "consolidate_folds in the output folder of the model first!\nThe folder you need to run this in is "
                  "%s" % model)


def predict_from_folder(model, input_folder, output_folder, folds, save_npz, num_threads_preprocessing, num_threads_nifti_save,
                        lowres_segmentations, part_id, num_parts, tta, mixed_precision=True, overwrite_existing=True,
                        mode='normal', overwrite_all_in_gpu=None, step_size=0.5, checkpoint_name="model_final_checkpoint",
                        segmentation_export_kwargs=None, disable_postprocessing=False):
    """reference :603-692: the standard naming -> predict_cases; the cases are strided over `num_parts` processes."""
    if mode in ('fast', 'fastest'):
        raise ValueError("mode %r is not available: its export resamples the label map instead of the probabilities, and the device "
                         "path needs neither shortcut; use 'normal'" % mode)
    if mode != 'normal':
        raise ValueError("unrecognized mode. Must be normal, fast or fastest")
    if lowres_segmentations is not None:
        raise NotImplementedError("cascade inputs (lowres_segmentations) are not on this path")
    os.makedirs(output_folder, exist_ok=True)
    assert os.path.isfile(os.path.join(model, "plans.pkl")), "Folder with saved model weights must contain a plans.pkl file"
    shutil.copy(os.path.join(model, 'plans.pkl'), output_folder)
    with open(os.path.join(model, "plans.pkl"), 'rb') as f:
        expected_num_modalities = pickle.load(f)['num_modalities']
    case_ids = check_input_folder_and_return_caseIDs(input_folder, expected_num_modalities)
    output_files = [os.path.join(output_folder, i + ".nii.gz") for i in case_ids]
    all_files = sorted(i for i in os.listdir(input_folder) if i.endswith(".nii.gz") and os.path.isfile(os.path.join(input_folder, i)))
    list_of_lists = [[os.path.join(input_folder, i) for i in all_files if i[:len(j)].startswith(j) and len(i) == (len(j) + 12)]
                     for j in case_ids]
    all_in_gpu = False if overwrite_all_in_gpu is None else overwrite_all_in_gpu
    return predict_cases(model, list_of_lists[part_id::num_parts], output_files[part_id::num_parts], folds, save_npz,
                         num_threads_preprocessing, num_threads_nifti_save, None, tta, mixed_precision=mixed_precision,
                         overwrite_existing=overwrite_existing, all_in_gpu=all_in_gpu, step_size=step_size,
                         checkpoint_name=checkpoint_name, segmentation_export_kwargs=segmentation_export_kwargs,
                         disable_postprocessing=disable_postprocessing)
