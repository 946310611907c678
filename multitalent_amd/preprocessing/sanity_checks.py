"""`verify_dataset_integrity` (reference preprocessing/sanity_checks.py:25-247): is a raw task folder what the pipeline expects?
Same checks, messages and outcomes as the reference, in two halves.

  structure pass   host only: `dataset.json`, the files of every listed case, stragglers, the label declaration, the geometry
                   headers of each case's files (the reference's `np.isclose` tolerances), the test set, the axis codes.
                   `verify_dataset_structure(folder)` runs it alone.
  voxel pass       on the device, while each case is in memory for the structure pass (a file is read once): the set of label
                   values is `mt_label_presence` (one pass, labels -1..1022; it flags a fraction, a NaN or a label outside that
                   range, and only such a case is then looked at on the host with `np.unique`); NaNs in an image are a torch
                   reduction on the uploaded volume.  This replaces the reference's `np.unique` per label file in a process
                   pool.  Without a HIP device `verify_dataset_integrity` raises; there is no CPU fallback.

Outcomes: AssertionError for missing files, stragglers, labels that are not 0, 1, 2, ... and unexpected label values (the message
names the files and the values); RuntimeError for a case listed twice; `raise Warning(...)` at the end for a geometry mismatch;
NaNs only print (the reference's changed default, :242-246)."""
import json
import os

import numpy as np
import torch

from .. import ops
from ..utilities.nifti_io import read_image

_LPS_TO_RAS = np.diag([-1.0, -1.0, 1.0])
_AXIS_LABELS = (('L', 'R'), ('P', 'A'), ('I', 'S'))
_TORCH_DTYPES = ('uint8', 'int8', 'int16', 'int32', 'int64', 'float32', 'float64')


def _nii_files(folder):
    return sorted(f for f in os.listdir(folder) if f.endswith(".nii.gz") and os.path.isfile(os.path.join(folder, f)))


def axis_codes(direction):
    """nibabel's `aff2axcodes` for the affine of an image with the ITK direction cosines `direction` (row-major 3x3, LPS): per
    voxel axis (x, y, z) the letter of the anatomical direction it runs towards.  Each voxel axis in turn takes the world axis
    along which it is longest, among the world axes no earlier voxel axis took.  The cosines are orthonormal, so nibabel's polar
    decomposition of the affine changes nothing and is left out, and the spacing scales whole columns and cannot change an
    argmax."""
    R = _LPS_TO_RAS @ np.array(direction, dtype=np.float64).reshape(3, 3)
    codes = []
    for in_ax in range(3):
        col = R[:, in_ax]
        if np.allclose(col, 0):
            codes.append(None)
            continue
        out_ax = int(np.argmax(np.abs(col)))
        codes.append(_AXIS_LABELS[out_ax][0 if col[out_ax] < 0 else 1])
        R[out_ax, :] = 0
    return tuple(codes)


def verify_all_same_orientation(folder, directions=None):
    """-> (all images of `folder` have the same axis codes, the distinct codes).  directions: the cosines of the files where the
    caller has read them already."""
    if directions is None:
        directions = [read_image(os.path.join(folder, n)).GetDirection() for n in _nii_files(folder)]
    orientations = np.array([axis_codes(d) for d in directions])
    unique_orientations = np.unique(orientations, axis=0) if len(orientations) else orientations
    return len(unique_orientations) == 1, unique_orientations


def verify_same_geometry(img_1, img_2):
    """img_*: `nifti_io.Image` or SimpleITK images."""
    ori1, spacing1, direction1, size1 = img_1.GetOrigin(), img_1.GetSpacing(), img_1.GetDirection(), img_1.GetSize()
    ori2, spacing2, direction2, size2 = img_2.GetOrigin(), img_2.GetSpacing(), img_2.GetDirection(), img_2.GetSize()
    same = True
    for what, a, b, tol in (("origin does not match between the images:", ori1, ori2, dict(rtol=1e-3, atol=1e-3)),
                            ("spacing does not match between the images", spacing1, spacing2, dict()),
                            ("direction does not match between the images", direction1, direction2, dict(rtol=1e-3)),
                            ("size does not match between the images", size1, size2, dict(rtol=1e-3))):
        if not np.all(np.isclose(a, b, **tol)):
            print("the " + what)
            print(a)
            print(b)
            same = False
    return same


def _upload(array):
    """-> float32 device tensor; the conversion runs on the device for every dtype torch can hold."""
    array = np.ascontiguousarray(array)
    if array.dtype.name in _TORCH_DTYPES:
        return torch.from_numpy(array).cuda().float().contiguous()
    return torch.from_numpy(array.astype(np.float32)).cuda()


def _device_voxel_check(label_file, label, image_files, images):
    """-> (label values as np.unique would list them, NaNs in the label map, per image: NaNs in it)."""
    try:
        values = ops.label_presence(_upload(label.array), "the label file %s" % label_file)
        label_nan = False
    except ValueError:                  # the flag of mt_label_presence: this one case is looked at on the host
        values = np.unique(np.asarray(label.array))
        label_nan = bool(np.any(np.isnan(values)))
    image_nans = []
    for img in images:
        a = np.asarray(img.array)
        image_nans.append(bool(torch.isnan(_upload(a)).any().item()) if a.dtype.kind == 'f' else False)
    return values, label_nan, image_nans


def _verify(folder, voxel_check):
    assert os.path.isfile(os.path.join(folder, "dataset.json")), "There needs to be a dataset.json file in folder, folder=%s" % folder
    assert os.path.isdir(os.path.join(folder, "imagesTr")), "There needs to be a imagesTr subfolder in folder, folder=%s" % folder
    assert os.path.isdir(os.path.join(folder, "labelsTr")), "There needs to be a labelsTr subfolder in folder, folder=%s" % folder
    with open(os.path.join(folder, "dataset.json")) as f:
        dataset = json.load(f)
    training_cases = dataset['training']
    num_modalities = len(dataset['modality'].keys())
    test_cases = dataset['test']
    expected_train_identifiers = [i['image'].split("/")[-1][:-7] for i in training_cases]
    expected_test_identifiers = [i.split("/")[-1][:-7] for i in test_cases]

    nii_files_in_imagesTr = _nii_files(os.path.join(folder, "imagesTr"))
    nii_files_in_labelsTr = _nii_files(os.path.join(folder, "labelsTr"))

    label_files, label_values, directions = [], [], {}
    geometries_OK = True
    has_nan = False

    if len(expected_train_identifiers) != len(np.unique(expected_train_identifiers)):
        raise RuntimeError("found duplicate training cases in dataset.json")

    print("Verifying training set")
    for c in expected_train_identifiers:
        print("checking case", c)
        expected_label_file = os.path.join(folder, "labelsTr", c + ".nii.gz")
        label_files.append(expected_label_file)
        expected_image_files = [os.path.join(folder, "imagesTr", c + "_%04.0d.nii.gz" % i) for i in range(num_modalities)]
        assert os.path.isfile(expected_label_file), "could not find label file for case %s. Expected file: \n%s" % (
            c, expected_label_file)
        assert all([os.path.isfile(i) for i in expected_image_files]), \
            "some image files are missing for case %s. Expected files:\n %s" % (c, expected_image_files)

        label = read_image(expected_label_file)
        images = [read_image(i) for i in expected_image_files]
        if voxel_check is not None:
            values, nans_in_seg, nans_in_images = voxel_check(expected_label_file, label, expected_image_files, images)
            label_values.append(values)
        else:
            nans_in_seg, nans_in_images = False, [False] * len(images)
        has_nan = has_nan | nans_in_seg
        if nans_in_seg:
            print("There are NAN values in segmentation %s" % expected_label_file)
        for i, img in enumerate(images):
            has_nan = has_nan | nans_in_images[i]
            directions[os.path.basename(expected_image_files[i])] = img.GetDirection()
            if not verify_same_geometry(img, label):
                geometries_OK = False
                print("The geometry of the image %s does not match the geometry of the label file. The pixel arrays "
                      "will not be aligned and nnU-Net cannot use this data. Please make sure your image modalities "
                      "are coregistered and have the same geometry as the label" % expected_image_files[0][:-12])
            if nans_in_images[i]:
                print("There are NAN values in image %s" % expected_image_files[i])
        del label, images

        for i in expected_image_files:
            nii_files_in_imagesTr.remove(os.path.basename(i))
        nii_files_in_labelsTr.remove(os.path.basename(expected_label_file))

    assert len(nii_files_in_imagesTr) == 0, \
        "there are training cases in imagesTr that are not listed in dataset.json: %s" % nii_files_in_imagesTr
    assert len(nii_files_in_labelsTr) == 0, \
        "there are training cases in labelsTr that are not listed in dataset.json: %s" % nii_files_in_labelsTr

    print("Verifying label values")
    expected_labels = list(int(i) for i in dataset['labels'].keys())
    if folder.split('/')[-1].startswith('Task128'):          # the reference's exception for this task: 0 is not declared there
        expected_labels = [0] + expected_labels
    expected_labels.sort()
    assert expected_labels[0] == 0, 'The first label must be 0 and maps to the background'
    labels_valid_consecutive = np.ediff1d(expected_labels) == 1
    assert all(labels_valid_consecutive), \
        f'Labels must be in consecutive order (0, 1, 2, ...). The labels ' \
        f'{np.array(expected_labels)[1:][~labels_valid_consecutive]} do not satisfy this restriction'

    if voxel_check is not None:
        print("Expected label values are", expected_labels)
        failed = []
        for fname, values in zip(label_files, label_values):
            invalid = [i for i in values if i not in expected_labels]
            if len(invalid) > 0:
                print("Unexpected labels found in file %s. Found these unexpected values (they should not be there) %s" % (
                    fname, invalid))
                failed.append("%s: %s" % (fname, invalid))
        if failed:
            raise AssertionError("Found unexpected labels in the training dataset. Please correct that or adjust your "
                                 "dataset.json accordingly\n" + "\n".join(failed))
        print("Labels OK")

    if len(expected_test_identifiers) > 0:
        print("Verifying test set")
        nii_files_in_imagesTs = _nii_files(os.path.join(folder, "imagesTs"))
        for c in expected_test_identifiers:
            expected_image_files = [os.path.join(folder, "imagesTs", c + "_%04.0d.nii.gz" % i) for i in range(num_modalities)]
            assert all([os.path.isfile(i) for i in expected_image_files]), \
                "some image files are missing for case %s. Expected files:\n %s" % (c, expected_image_files)
            if num_modalities > 1:
                images = [read_image(i) for i in expected_image_files]
                for i, img in enumerate(images[1:]):
                    assert verify_same_geometry(img, images[0]), "The modalities of the image %s do not seem to be " \
                                                                 "registered. Please coregister your modalities." % (
                                                                     expected_image_files[i])
            for i in expected_image_files:
                nii_files_in_imagesTs.remove(os.path.basename(i))
        assert len(nii_files_in_imagesTs) == 0, \
            "there are training cases in imagesTs that are not listed in dataset.json: %s" % nii_files_in_imagesTs

    all_same, unique_orientations = verify_all_same_orientation(os.path.join(folder, "imagesTr"),
                                                                [directions[k] for k in sorted(directions)])
    if not all_same:
        print("WARNING: Not all images in the dataset have the same axis ordering. We very strongly recommend you correct "
              "that by reorienting the data. fslreorient2std should do the trick")
    if not geometries_OK:
        raise Warning("GEOMETRY MISMATCH FOUND! CHECK THE TEXT OUTPUT! This does not cause an error at this point  but you "
                      "should definitely check whether your geometries are alright!")
    else:
        print("Dataset OK")
    if has_nan:
        print("Some images have nan values in them. This will break the training. See text output above to see which ones")


def verify_dataset_structure(folder):
    """The host half alone: everything `verify_dataset_integrity` checks except the voxel values (label sets, NaNs)."""
    _verify(folder, None)


def verify_dataset_integrity(folder):
    """folder: a raw task folder with `dataset.json`, `imagesTr`, `labelsTr` (and `imagesTs` where a test set is listed)."""
    if not torch.cuda.is_available():
        raise RuntimeError("multitalent_amd: the voxel pass of verify_dataset_integrity runs on a HIP device only; there is no "
                           "CPU fallback (verify_dataset_structure is the host half)")
    _verify(folder, _device_voxel_check)
