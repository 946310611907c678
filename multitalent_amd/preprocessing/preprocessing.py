"""`GenericPreprocessor` (reference preprocessing/preprocessing.py:200-399).  Test time (`preprocess_patient` of the trainers): read
the files on the host, then crop to the non-zero region (`device_cropping`: `mt_nonzero_mask`, `mt_fill_holes3d`,
`mt_crop_nonzero`), resample to the plan's spacing and normalise ON THE DEVICE (`device_preprocessing`: `mt_spline_prefilter3` +
`mt_affine_sample`).  Training cases (`run` / `_run_internal` / `preprocess_training_case`): the cropped case is resampled with its
label map (order 1 per label, `mt_affine_sample` mode 11), normalised with any of the schemes "CT", "CT2", "noNorm" and the
per-case z-score, each with or without `use_mask_for_norm` (`mt_masked_moments`, `mt_intensity_normalize`), and its class locations
are sampled (`mt_label_counts`, `mt_label_locations`); the host reads and writes the files.  There is no CPU fallback.
`GenericPreprocessor_linearResampling` (preprocessing.py:402-407) and `Preprocessor3DDifferentResampling` (:410-491) differ in the
resampling orders alone and take them to the resize unit (`device_preprocessing.resample_data_or_seg`); `PREPROCESSORS` names the
classes a plans file may ask for."""
import os
import pickle
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops
from . import device_cropping
from .cropping import ImageCropper, load_case_from_list_of_files
from . import device_preprocessing as dp
from .device_preprocessing import resample_and_normalize_ct

RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD = 3


class GenericPreprocessor(object):
    def __init__(self, normalization_scheme_per_modality, use_nonzero_mask, transpose_forward, intensityproperties=None):
        self.transpose_forward = list(transpose_forward)
        self.intensityproperties = intensityproperties
        self.normalization_scheme_per_modality = normalization_scheme_per_modality
        self.use_nonzero_mask = use_nonzero_mask
        self.resample_separate_z_anisotropy_threshold = RESAMPLING_SEPARATE_Z_ANISO_THRESHOLD
        self.resample_order_data = 3
        self.resample_order_seg = 1

    @staticmethod
    def load_cropped(cropped_output_dir, case_identifier):
        fname = os.path.join(cropped_output_dir, "%s.npz" % case_identifier)
        if torch.cuda.is_available():        # inflated on the device (utilities.npz_io.load_npz_device): device tensors
            from ..utilities.npz_io import load_npz_device
            all_data = load_npz_device(fname, 'data', torch.device('cuda', torch.cuda.current_device()))
            data = all_data[:-1].float()
        else:
            all_data = np.load(fname)['data']
            data = all_data[:-1].astype(np.float32)
        seg = all_data[-1:]
        with open(os.path.join(cropped_output_dir, "%s.pkl" % case_identifier), 'rb') as f:
            properties = pickle.load(f)
        return data, seg, properties

    def resample_and_normalize(self, data, target_spacing, properties, seg=None, force_separate_z=None, return_device=False,
                               keep_seg=False):
        """preprocessing.py:226-311.  `data` / `seg` are already transposed, `properties['original_spacing']` is not.
        The "CT" scheme without `use_mask_for_norm` and without `keep_seg` is the test-time path: the returned seg (the -1 / 0
        non-zero mask, which no caller on that path reads) is resampled with nearest neighbour: the same index gather on the host
        for a numpy seg and in torch for a device tensor.  Any other scheme, a `use_mask_for_norm`, or `keep_seg=True` (the seg is
        a label map to be kept: training cases) takes the full path of the reference: the seg is resampled per label with order 1
        and every scheme is available.  A tensor stays on the device with `return_device=True` and comes back as numpy otherwise."""
        schemes = [self.normalization_scheme_per_modality[c] for c in range(len(data))]
        use_mask = [bool(self.use_nonzero_mask[c]) for c in range(len(data))]
        if keep_seg or any(s != "CT" for s in schemes) or any(use_mask):
            return self._resample_and_normalize_full(data, target_spacing, properties, seg, force_separate_z, return_device, schemes,
                                                     use_mask)
        assert self.intensityproperties is not None, "ERROR: if there is a CT then we need intensity properties"
        spacing = np.array(properties["original_spacing"])[self.transpose_forward]
        out = resample_and_normalize_ct(data, spacing, target_spacing, self.intensityproperties, force_separate_z,
                                        self.resample_separate_z_anisotropy_threshold)
        new_shape = tuple(int(i) for i in out.shape[1:])
        if seg is not None and tuple(seg.shape[1:]) != new_shape:
            idx = [np.clip(np.floor((np.arange(n) + 0.5) * (o / n)).astype(int), 0, o - 1) for n, o in zip(new_shape, seg.shape[1:])]
            if torch.is_tensor(seg):
                for a in range(3):
                    seg = seg.index_select(a + 1, torch.from_numpy(idx[a].astype(np.int64)).to(seg.device))
            else:
                seg = seg[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]]
        if seg is not None:
            seg[seg < -1] = 0
            if torch.is_tensor(seg) and not return_device:
                seg = seg.cpu().numpy()
        properties["size_after_resampling"] = new_shape
        properties["spacing_after_resampling"] = target_spacing
        return (out if return_device else out.cpu().numpy()), seg, properties

    def _resample_and_normalize_full(self, data, target_spacing, properties, seg, force_separate_z, return_device, schemes, use_mask):
        assert len(self.normalization_scheme_per_modality) == len(data), "self.normalization_scheme_per_modality must have as many " \
                                                                         "entries as data has modalities"
        assert len(self.use_nonzero_mask) == len(data), "self.use_nonzero_mask must have as many entries as data has modalities"
        if any(use_mask) and seg is None:
            raise ValueError("use_mask_for_norm needs the segmentation of the cropped case (its -1 marks the outside of the non-zero mask)")
        spacing = np.array(properties["original_spacing"])[self.transpose_forward]
        data = dp._to_device(data).float()
        data = torch.nan_to_num(data, nan=0.0, posinf=None, neginf=None) if torch.isnan(data).any() else data
        new_shape, sep, axis = dp.resampling_plan(data.shape[1:], spacing, target_spacing, force_separate_z,
                                                  self.resample_separate_z_anisotropy_threshold)
        seg_in = dp._to_device(seg).float() if seg is not None else None
        out, seg = self._resample(data, seg_in, new_shape, axis, sep)
        out = out.clone() if out is data else out.contiguous()
        if seg is not None:
            seg = seg.clone() if seg is seg_in else seg
            seg[seg < -1] = 0
        properties["size_after_resampling"] = tuple(int(i) for i in out.shape[1:])
        properties["spacing_after_resampling"] = target_spacing
        dp.normalize(out, seg, schemes, use_mask, self.intensityproperties)
        if not return_device:
            out, seg = out.cpu().numpy(), (seg.cpu().numpy() if seg is not None else None)
        return out, seg, properties

    def _resample(self, data, seg, new_shape, axis, sep):
        """The resampling of the full path: float32 device tensors [C, X, Y, Z] (seg may be None) -> the same at `new_shape`.  Here
        order 3 / z 0 for the data and order 1 / z 0 for the labels, on `mt_spline_prefilter3` + `mt_affine_sample`."""
        return dp.resample_data(data, new_shape, axis, sep), (dp.resample_seg(seg, new_shape, axis, sep) if seg is not None else None)

    def preprocess_test_case(self, data_files, target_spacing, seg_file=None, force_separate_z=None, return_device=False):
        """preprocessing.py:313-321.  The uncropped float32 volume is uploaded once and cropped on the device; a volume beyond the
        int32 index range of the device labelling goes through the host cropper."""
        data, seg, properties = load_case_from_list_of_files(data_files, seg_file)
        perm = (0, *[i + 1 for i in self.transpose_forward])
        if int(np.prod(data.shape[1:], dtype=np.int64)) > ops.CROP_MAX_VOXELS:
            print("preprocess_test_case: %d voxels exceed the device cropper's int32 range, cropping on the host"
                  % int(np.prod(data.shape[1:], dtype=np.int64)))
            data, seg, properties = ImageCropper.crop(data, properties, seg)
            data, seg = data.transpose(perm), seg.transpose(perm)
        else:
            data, seg, properties = device_cropping.ImageCropper.crop(data, properties, seg)
            data, seg = data.permute(perm).contiguous(), seg.permute(perm).contiguous()
        data, seg, properties = self.resample_and_normalize(data, target_spacing, properties, seg, force_separate_z, return_device)
        if not torch.is_tensor(data):
            data = data.astype(np.float32)
        return data, seg, properties

    def preprocess_training_case(self, data, seg, properties, target_spacing, all_classes, force_separate_z=None):
        """`_run_internal` between its file accesses (preprocessing.py:327-353): data [C, X, Y, Z] and seg [1, X, Y, Z] of a cropped
        case (numpy or device tensors, not yet transposed) -> (all_data, properties): the float32 device tensor [C + 1, X', Y', Z']
        that `<case>.npz` holds (seg last) and the properties with `class_locations`, `size_after_resampling` and
        `spacing_after_resampling`."""
        if not torch.cuda.is_available():
            raise RuntimeError("multitalent_amd: training-case preprocessing runs on a HIP device only; there is no CPU fallback")
        perm = (0, *[i + 1 for i in self.transpose_forward])
        data, seg = dp._to_device(data).permute(perm).contiguous(), dp._to_device(seg).permute(perm).contiguous()
        data, seg, properties = self.resample_and_normalize(data, target_spacing, properties, seg, force_separate_z, return_device=True,
                                                            keep_seg=True)
        all_data = torch.cat((data, seg.float()), 0)
        properties['class_locations'] = dp.class_locations(all_data[-1], all_classes)
        return all_data, properties

    @staticmethod
    def _save_case(output_folder_stage, case_identifier, all_data, properties):
        """all_data: the float32 device tensor (compressed on the device, utilities.npz_io), the members `encode_npz_device` made
        of it (only the file is written here), or a host array (numpy's writer, as before)."""
        from ..utilities import npz_io
        fname = os.path.join(output_folder_stage, "%s.npz" % case_identifier)
        if isinstance(all_data, list):
            npz_io.write_npz_members(fname, all_data)
        elif torch.is_tensor(all_data) and all_data.is_cuda:
            npz_io.save_npz_device(fname, data=all_data)
        else:
            np.savez_compressed(fname, data=all_data)
        with open(os.path.join(output_folder_stage, "%s.pkl" % case_identifier), 'wb') as f:
            pickle.dump(properties, f)

    def _run_internal(self, target_spacing, case_identifier, output_folder_stage, cropped_output_dir, force_separate_z, all_classes):
        """preprocessing.py:323-359: `<case>.npz` (key `data`, float32 [C + 1, X, Y, Z]) and `<case>.pkl` in `output_folder_stage`."""
        self._run_case(target_spacing, case_identifier, output_folder_stage, cropped_output_dir, force_separate_z, all_classes, None)

    def _run_case(self, target_spacing, case_identifier, output_folder_stage, cropped_output_dir, force_separate_z, all_classes, writer):
        """writer: None, or an executor that takes the file writes off this thread (`run`); the case is compressed on the device,
        from this thread, and only its compressed bytes wait for the executor."""
        if not torch.cuda.is_available():
            raise RuntimeError("multitalent_amd: training-case preprocessing runs on a HIP device only; there is no CPU fallback")
        data, seg, properties = self.load_cropped(cropped_output_dir, case_identifier)
        all_data, properties = self.preprocess_training_case(data, seg, properties, target_spacing, all_classes, force_separate_z)
        all_data = all_data.float()
        print("saving: ", os.path.join(output_folder_stage, "%s.npz" % case_identifier))
        if writer is None:
            self._save_case(output_folder_stage, case_identifier, all_data, properties)
            return None
        from ..utilities.npz_io import encode_npz_device
        return writer.submit(self._save_case, output_folder_stage, case_identifier, encode_npz_device(data=all_data), properties)

    def run(self, target_spacings, input_folder_with_cropped_npz, output_folder, data_identifier, num_threads=8, force_separate_z=None):
        """preprocessing.py:361-399: every cropped case of `input_folder_with_cropped_npz` into `<data_identifier>_stage<i>` per
        target spacing.  The cases go through the one device in sequence; `num_threads` (a number or one per stage) sizes the host
        pool that writes the `.npz` files, which the device compresses, behind it."""
        if not torch.cuda.is_available():
            raise RuntimeError("multitalent_amd: training-case preprocessing runs on a HIP device only; there is no CPU fallback")
        print("Initializing to run preprocessing")
        print("npz folder:", input_folder_with_cropped_npz)
        print("output_folder:", output_folder)
        cases = sorted(f[:-4] for f in os.listdir(input_folder_with_cropped_npz) if f.endswith(".npz"))
        os.makedirs(output_folder, exist_ok=True)
        num_stages = len(target_spacings)
        if not isinstance(num_threads, (list, tuple, np.ndarray)):
            num_threads = [num_threads] * num_stages
        assert len(num_threads) == num_stages
        with open(os.path.join(input_folder_with_cropped_npz, 'dataset_properties.pkl'), 'rb') as f:
            all_classes = pickle.load(f)['all_classes']
        for i in range(num_stages):
            output_folder_stage = os.path.join(output_folder, data_identifier + "_stage%d" % i)
            os.makedirs(output_folder_stage, exist_ok=True)
            with ThreadPoolExecutor(max_workers=max(1, int(num_threads[i]))) as writer:
                pending = []
                for case in cases:
                    pending.append(self._run_case(target_spacings[i], case, output_folder_stage, input_folder_with_cropped_npz,
                                                  force_separate_z, all_classes, writer))
                    while len(pending) > 2 * max(1, int(num_threads[i])):          # bounds the volumes waiting in host memory
                        pending.pop(0).result()
                for p in pending:
                    p.result()


class _ResizeUnitPreprocessor(GenericPreprocessor):
    """A preprocessor whose resampling orders differ from the default's: every case takes the full path of the reference's
    `resample_and_normalize` (the label map or non-zero mask is resampled by the label rule, every scheme is available), and the
    resampling is `device_preprocessing.resample_data_or_seg` on the resize unit (`mt_resize_prefilter3`, `mt_resize`,
    `mt_resize_labels`, `mt_resize_labels_axis`) with the orders of the class."""
    resample_order_z_data = 0
    resample_order_z_seg = 0

    def resample_and_normalize(self, data, target_spacing, properties, seg=None, force_separate_z=None, return_device=False,
                               keep_seg=False):
        schemes = [self.normalization_scheme_per_modality[c] for c in range(len(data))]
        use_mask = [bool(self.use_nonzero_mask[c]) for c in range(len(data))]
        return self._resample_and_normalize_full(data, target_spacing, properties, seg, force_separate_z, return_device, schemes,
                                                 use_mask)

    def _resample(self, data, seg, new_shape, axis, sep):
        out = dp.resample_data_or_seg(data, new_shape, False, axis, self.resample_order_data, sep, self.resample_order_z_data)
        if seg is not None:
            seg = dp.resample_data_or_seg(seg, new_shape, True, axis, self.resample_order_seg, sep, self.resample_order_z_seg)
        return out, seg


class GenericPreprocessor_linearResampling(_ResizeUnitPreprocessor):
    """preprocessing.py:402-407: order 1 for the data and for the labels, order 0 along a separately resampled axis."""

    def __init__(self, normalization_scheme_per_modality, use_nonzero_mask, transpose_forward, intensityproperties=None):
        super().__init__(normalization_scheme_per_modality, use_nonzero_mask, transpose_forward, intensityproperties)
        self.resample_order_data = 1
        self.resample_order_seg = 1


class Preprocessor3DDifferentResampling(_ResizeUnitPreprocessor):
    """preprocessing.py:410-491 (the preprocessor of `ExperimentPlanner3D_v23`): order 3 for the data and order 1 for the labels,
    and along a separately resampled axis order 3 for the data and order 1 for the labels where the default takes order 0."""
    resample_order_z_data = 3
    resample_order_z_seg = 1


PREPROCESSORS = ("GenericPreprocessor", "GenericPreprocessor_linearResampling", "Preprocessor3DDifferentResampling")
