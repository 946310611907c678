"""`ExperimentPlanner` (reference experiment_planning/experiment_planner_baseline_3DUNet.py:32-444): from the fingerprint of a
cropped dataset (`dataset_properties.pkl`, written by `DatasetAnalyzer`) to the plans file the trainers read — target spacing,
transposition, per stage the patch size, batch size and the network topology, and the normalisation schemes — and on to the
preprocessed training cases through `GenericPreprocessor.run`, which works on the device.

Planning is float64 and integer arithmetic on a few numbers per case and stays on the host.  The plans are compared with the
reference's for equality (tests/golden/planning.json), so the numpy calls and their order are the reference's.  The reference
states `get_properties_for_stage` once per planner; here it is stated once, and a planner overrides the three things in which
the planners differ: `topology` (how the axes are pooled), `vram_budget` and `vram_estimate`."""
import os
import pickle
import shutil
from collections import OrderedDict
from copy import deepcopy

import numpy as np

import multitalent_amd
from ..network_architecture.generic_UNet import Generic_UNet
from ..paths import default_data_identifier, default_num_threads
from ..training.model_restore import recursive_find_python_class
from .common_utils import get_pool_and_conv_props_poolLateV2


def _load_pickle(fname):
    with open(fname, 'rb') as f:
        return pickle.load(f)


class ExperimentPlanner(object):
    def __init__(self, folder_with_cropped_data, preprocessed_output_folder):
        self.folder_with_cropped_data = folder_with_cropped_data
        self.preprocessed_output_folder = preprocessed_output_folder
        self.list_of_cropped_npz_files = [os.path.join(folder_with_cropped_data, i) for i in sorted(
            f for f in os.listdir(folder_with_cropped_data)
            if f.endswith(".npz") and os.path.isfile(os.path.join(folder_with_cropped_data, f)))]
        self.preprocessor_name = "GenericPreprocessor"
        assert os.path.isfile(os.path.join(self.folder_with_cropped_data, "dataset_properties.pkl")), \
            "folder_with_cropped_data must contain dataset_properties.pkl"
        self.dataset_properties = _load_pickle(os.path.join(self.folder_with_cropped_data, "dataset_properties.pkl"))

        self.plans_per_stage = OrderedDict()
        self.plans = OrderedDict()
        self.plans_fname = os.path.join(self.preprocessed_output_folder, "nnUNetPlans" + "fixed_plans_3D.pkl")
        self.data_identifier = default_data_identifier

        self.transpose_forward = [0, 1, 2]
        self.transpose_backward = [0, 1, 2]

        self.unet_base_num_features = Generic_UNet.BASE_NUM_FEATURES_3D
        self.unet_max_num_filters = 320
        self.unet_max_numpool = 999
        self.unet_min_batch_size = 2
        self.unet_featuremap_min_edge_length = 4

        self.target_spacing_percentile = 50
        self.anisotropy_threshold = 3
        self.how_much_of_a_patient_must_the_network_see_at_stage0 = 4      # the patch covers at least 1/4 of the median case
        self.batch_size_covers_max_percent_of_dataset = 0.05               # one batch covers at most 5 % of the dataset's voxels
        self.conv_per_stage = 2

    # ---- the fingerprint ---------------------------------------------------------------------------------------------------
    def get_target_spacing(self):
        return np.percentile(np.vstack(self.dataset_properties['all_spacings']), self.target_spacing_percentile, 0)

    def save_my_plans(self):
        with open(self.plans_fname, 'wb') as f:
            pickle.dump(self.plans, f)

    def load_my_plans(self):
        self.plans = _load_pickle(self.plans_fname)
        self.plans_per_stage = self.plans['plans_per_stage']
        self.dataset_properties = self.plans['dataset_properties']
        self.transpose_forward = self.plans['transpose_forward']
        self.transpose_backward = self.plans['transpose_backward']

    # ---- what the planners differ in ---------------------------------------------------------------------------------------
    def topology(self, spacing, patch_size):
        """-> num_pool_per_axis, pool kernels, conv kernels, padded patch size, what each axis must be divisible by."""
        return get_pool_and_conv_props_poolLateV2(patch_size, self.unet_featuremap_min_edge_length, self.unet_max_numpool, spacing)

    def vram_budget(self):
        return Generic_UNet.use_this_for_batch_size_computation_3D

    def vram_estimate(self, patch_size, num_pool_per_axis, pool_op_kernel_sizes, num_modalities, num_classes):
        return Generic_UNet.compute_approx_vram_consumption(patch_size, num_pool_per_axis, self.unet_base_num_features,
                                                            self.unet_max_num_filters, num_modalities, num_classes,
                                                            pool_op_kernel_sizes, conv_per_stage=self.conv_per_stage)

    def default_batch_size(self):
        return Generic_UNet.DEFAULT_BATCH_SIZE_3D

    # ---- one stage ---------------------------------------------------------------------------------------------------------
    def _median_shape_and_first_patch(self, current_spacing, original_spacing, original_shape):
        """-> the median shape at `current_spacing`, and the patch the search starts from: isotropic in millimetres (512 mm along
        the finest axis), clipped to the median shape."""
        new_median_shape = np.round(original_spacing / current_spacing * original_shape).astype(int)
        input_patch_size = 1 / np.array(current_spacing)                  # voxels per millimetre
        input_patch_size /= input_patch_size.mean()
        input_patch_size *= 1 / min(input_patch_size) * 512
        input_patch_size = np.round(input_patch_size).astype(int)
        return new_median_shape, [min(i, j) for i, j in zip(input_patch_size, new_median_shape)]

    def _shrink(self, current_spacing, new_shp, new_median_shape, shape_must_be_divisible_by):
        """One step of the search: the axis that is largest relative to the median shape loses one multiple of its divisor (the
        divisor the SMALLER patch would have); -> the topology of the result."""
        axis_to_be_reduced = np.argsort(new_shp / new_median_shape)[-1]
        tmp = deepcopy(new_shp)
        tmp[axis_to_be_reduced] -= shape_must_be_divisible_by[axis_to_be_reduced]
        shape_must_be_divisible_by_new = self.topology(current_spacing, tmp)[4]
        new_shp[axis_to_be_reduced] -= shape_must_be_divisible_by_new[axis_to_be_reduced]
        return self.topology(current_spacing, new_shp)

    def _batch_size(self, ref, here, minimum, new_median_shape, num_cases, input_patch_size):
        dataset_num_voxels = np.prod(new_median_shape) * num_cases
        batch_size = int(np.floor(max(ref / here, 1) * minimum))
        max_batch_size = np.round(self.batch_size_covers_max_percent_of_dataset * dataset_num_voxels /
                                  np.prod(input_patch_size, dtype=np.int64)).astype(int)
        max_batch_size = max(max_batch_size, self.unet_min_batch_size)
        return max(1, min(batch_size, max_batch_size))

    def _stage_plan(self, batch_size, num_pool_per_axis, patch_size, median_shape, current_spacing, original_spacing,
                    pool_op_kernel_sizes, conv_kernel_sizes):
        return {
            'batch_size': batch_size,
            'num_pool_per_axis': num_pool_per_axis,
            'patch_size': patch_size,
            'median_patient_size_in_voxels': median_shape,
            'current_spacing': current_spacing,
            'original_spacing': original_spacing,
            'do_dummy_2D_data_aug': (max(patch_size) / patch_size[0]) > self.anisotropy_threshold,
            'pool_op_kernel_sizes': pool_op_kernel_sizes,
            'conv_kernel_sizes': conv_kernel_sizes,
        }

    def get_properties_for_stage(self, current_spacing, original_spacing, original_shape, num_cases, num_modalities, num_classes):
        """The patch starts isotropic in millimetres, clipped to the median shape of the dataset at this spacing, and shrinks
        until the network's estimate fits the budget; what is left of the budget goes into the batch size."""
        new_median_shape, input_patch_size = self._median_shape_and_first_patch(current_spacing, original_spacing, original_shape)
        num_pool_per_axis, pool_kernels, conv_kernels, new_shp, divisible_by = self.topology(current_spacing, input_patch_size)
        ref = self.vram_budget()
        here = self.vram_estimate(new_shp, num_pool_per_axis, pool_kernels, num_modalities, num_classes)
        while here > ref:
            num_pool_per_axis, pool_kernels, conv_kernels, new_shp, divisible_by = \
                self._shrink(current_spacing, new_shp, new_median_shape, divisible_by)
            here = self.vram_estimate(new_shp, num_pool_per_axis, pool_kernels, num_modalities, num_classes)
        batch_size = self._batch_size(ref, here, self.default_batch_size(), new_median_shape, num_cases, new_shp)
        return self._stage_plan(batch_size, num_pool_per_axis, new_shp, new_median_shape, current_spacing, original_spacing,
                                pool_kernels, conv_kernels)

    # ---- the experiment ----------------------------------------------------------------------------------------------------
    def plan_experiment(self):
        use_nonzero_mask_for_normalization = self.determine_whether_to_use_mask_for_norm()
        print("Are we using the nonzero mask for normalization?", use_nonzero_mask_for_normalization)
        spacings = self.dataset_properties['all_spacings']
        sizes = self.dataset_properties['all_sizes']
        all_classes = self.dataset_properties['all_classes']
        modalities = self.dataset_properties['modalities']
        num_modalities = len(list(modalities.keys()))

        target_spacing = self.get_target_spacing()
        new_shapes = [np.array(i) / target_spacing * np.array(j) for i, j in zip(spacings, sizes)]

        # the coarsest axis goes first
        max_spacing_axis = np.argmax(target_spacing)
        remaining_axes = [i for i in list(range(3)) if i != max_spacing_axis]
        self.transpose_forward = [max_spacing_axis] + remaining_axes
        self.transpose_backward = [np.argwhere(np.array(self.transpose_forward) == i)[0][0] for i in range(3)]

        median_shape = np.median(np.vstack(new_shapes), 0)
        print("the median shape of the dataset is ", median_shape)
        print("the max shape in the dataset is ", np.max(np.vstack(new_shapes), 0))
        print("the min shape in the dataset is ", np.min(np.vstack(new_shapes), 0))
        print("we don't want feature maps smaller than ", self.unet_featuremap_min_edge_length, " in the bottleneck")

        self.plans_per_stage = list()
        target_spacing_transposed = np.array(target_spacing)[self.transpose_forward]
        median_shape_transposed = np.array(median_shape)[self.transpose_forward]
        print("the transposed median shape of the dataset is ", median_shape_transposed)
        num_cases = len(self.list_of_cropped_npz_files)

        print("generating configuration for 3d_fullres")
        self.plans_per_stage.append(self.get_properties_for_stage(target_spacing_transposed, target_spacing_transposed,
                                                                  median_shape_transposed, num_cases, num_modalities,
                                                                  len(all_classes) + 1))
        architecture_input_voxels_here = np.prod(self.plans_per_stage[-1]['patch_size'], dtype=np.int64)
        more = not (np.prod(median_shape) / architecture_input_voxels_here
                    < self.how_much_of_a_patient_must_the_network_see_at_stage0)
        if more:
            print("generating configuration for 3d_lowres")
            # the low-resolution stage: the spacing grows by 1 % a step (only the finer axes while one is more than twice as fine
            # as the coarsest) until the median case holds at most 4 patches of the plan that spacing gives
            lowres_stage_spacing = deepcopy(target_spacing)
            num_voxels = np.prod(median_shape, dtype=np.float64)
            while num_voxels > self.how_much_of_a_patient_must_the_network_see_at_stage0 * architecture_input_voxels_here:
                max_spacing = max(lowres_stage_spacing)
                if np.any((max_spacing / lowres_stage_spacing) > 2):
                    lowres_stage_spacing[(max_spacing / lowres_stage_spacing) > 2] *= 1.01
                else:
                    lowres_stage_spacing *= 1.01
                num_voxels = np.prod(target_spacing / lowres_stage_spacing * median_shape, dtype=np.float64)
                lowres_stage_spacing_transposed = np.array(lowres_stage_spacing)[self.transpose_forward]
                new = self.get_properties_for_stage(lowres_stage_spacing_transposed, target_spacing_transposed,
                                                    median_shape_transposed, num_cases, num_modalities, len(all_classes) + 1)
                architecture_input_voxels_here = np.prod(new['patch_size'], dtype=np.int64)
            # kept only where it holds less than half the voxels of the full-resolution stage
            if 2 * np.prod(new['median_patient_size_in_voxels'], dtype=np.int64) < np.prod(
                    self.plans_per_stage[0]['median_patient_size_in_voxels'], dtype=np.int64):
                self.plans_per_stage.append(new)

        self.plans_per_stage = self.plans_per_stage[::-1]
        self.plans_per_stage = {i: self.plans_per_stage[i] for i in range(len(self.plans_per_stage))}
        print(self.plans_per_stage)
        print("transpose forward", self.transpose_forward)
        print("transpose backward", self.transpose_backward)

        self.plans = {'num_stages': len(list(self.plans_per_stage.keys())), 'num_modalities': num_modalities,
                      'modalities': modalities, 'normalization_schemes': self.determine_normalization_scheme(),
                      'dataset_properties': self.dataset_properties, 'list_of_npz_files': self.list_of_cropped_npz_files,
                      'original_spacings': spacings, 'original_sizes': sizes,
                      'preprocessed_data_folder': self.preprocessed_output_folder, 'num_classes': len(all_classes),
                      'all_classes': all_classes, 'base_num_features': self.unet_base_num_features,
                      'use_mask_for_norm': use_nonzero_mask_for_normalization,
                      'keep_only_largest_region': None, 'min_region_size_per_class': None, 'min_size_per_class': None,
                      'transpose_forward': self.transpose_forward, 'transpose_backward': self.transpose_backward,
                      'data_identifier': self.data_identifier, 'plans_per_stage': self.plans_per_stage,
                      'preprocessor_name': self.preprocessor_name, 'conv_per_stage': self.conv_per_stage}
        self.save_my_plans()

    def determine_normalization_scheme(self):
        schemes = OrderedDict()
        modalities = self.dataset_properties['modalities']
        for i in range(len(list(modalities.keys()))):
            if modalities[i] == "CT" or modalities[i] == 'ct':
                schemes[i] = "CT"
            elif modalities[i] == 'noNorm':
                schemes[i] = "noNorm"
            else:
                schemes[i] = "nonCT"
        return schemes

    def save_properties_of_cropped(self, case_identifier, properties):
        with open(os.path.join(self.folder_with_cropped_data, "%s.pkl" % case_identifier), 'wb') as f:
            pickle.dump(properties, f)

    def load_properties_of_cropped(self, case_identifier):
        return _load_pickle(os.path.join(self.folder_with_cropped_data, "%s.pkl" % case_identifier))

    def _case_identifiers(self):
        return [os.path.basename(c)[:-4] for c in self.list_of_cropped_npz_files]

    def determine_whether_to_use_mask_for_norm(self):
        """A modality that is not CT is normalised inside the non-zero mask only where cropping to that mask shrank the median
        case to less than 3/4 (brain MRI); the decision is also written into every cropped `<case>.pkl`."""
        modalities = self.dataset_properties['modalities']
        use_nonzero_mask_for_norm = OrderedDict()
        for i in range(len(list(modalities.keys()))):
            if "CT" in modalities[i]:
                use_nonzero_mask_for_norm[i] = False
            else:
                all_size_reductions = [self.dataset_properties['size_reductions'][k]
                                       for k in self.dataset_properties['size_reductions'].keys()]
                if np.median(all_size_reductions) < 3 / 4.:
                    print("using nonzero mask for normalization")
                    use_nonzero_mask_for_norm[i] = True
                else:
                    print("not using nonzero mask for normalization")
                    use_nonzero_mask_for_norm[i] = False
        for case_identifier in self._case_identifiers():
            properties = self.load_properties_of_cropped(case_identifier)
            properties['use_nonzero_mask_for_norm'] = use_nonzero_mask_for_norm
            self.save_properties_of_cropped(case_identifier, properties)
        return use_nonzero_mask_for_norm

    def run_preprocessing(self, num_threads):
        """num_threads: a number, or (low resolution, full resolution); they size the host pools that write behind the device."""
        gt = os.path.join(self.preprocessed_output_folder, "gt_segmentations")
        if os.path.isdir(gt):
            shutil.rmtree(gt)
        shutil.copytree(os.path.join(self.folder_with_cropped_data, "gt_segmentations"), gt)
        folder = [os.path.join(multitalent_amd.__path__[0], "preprocessing")]
        preprocessor_class = recursive_find_python_class(folder, self.preprocessor_name, "multitalent_amd.preprocessing")
        assert preprocessor_class is not None
        preprocessor = preprocessor_class(self.plans['normalization_schemes'], self.plans['use_mask_for_norm'],
                                          self.transpose_forward, self.plans['dataset_properties']['intensityproperties'])
        target_spacings = [i["current_spacing"] for i in self.plans_per_stage.values()]
        if self.plans['num_stages'] > 1 and not isinstance(num_threads, (list, tuple)):
            num_threads = (default_num_threads, num_threads)
        elif self.plans['num_stages'] == 1 and isinstance(num_threads, (list, tuple)):
            num_threads = num_threads[-1]
        preprocessor.run(target_spacings, self.folder_with_cropped_data, self.preprocessed_output_folder,
                         self.plans['data_identifier'], num_threads)
