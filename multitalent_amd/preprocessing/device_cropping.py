"""Cropping a case to its non-zero region ON THE DEVICE: `preprocessing/cropping.py` (reference preprocessing/cropping.py:23-116,
139-150) with the same names and signatures, on device tensors.  numpy inputs are uploaded; results stay on the device.

  create_nonzero_mask   `mt_nonzero_mask` (any channel != 0, numpy's rule on the bit pattern) + `mt_fill_holes3d`
                        (scipy.ndimage.binary_fill_holes with its default structure: the 6-connected background components that
                        touch no face of the volume are filled; the union-find labelling of `mt_cc_label3d` does the work);
  crop_to_nonzero       the two above, ONE device-to-host read of the seven box integers `mt_fill_holes3d` reduces, then
                        `mt_crop_nonzero`: data and segmentation of the box in one pass.

  ImageCropper          the static `crop` / `crop_from_list_of_files` of a single case, and the offline cropper of a dataset
                        (reference cropping.py:119-216): `run_cropping` writes `<case>.npz` / `<case>.pkl` and `gt_segmentations/`;
                        `num_threads` host threads read the files and write the results, which the device compresses, and
                        `properties['classes']` comes from `mt_label_presence`.

There is no CPU labelling here: without a HIP device every function raises (the host path is `cropping.py`).  The data must be
float32 (what `load_case_from_list_of_files` returns), a given seg float32 too."""
import os
import pickle
import shutil
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops
from ..utilities.npz_io import encode_npz_device
from .cropping import get_case_identifier, load_case_from_list_of_files  # noqa: F401  (same public names as cropping.py)


def _no_device():
    raise RuntimeError("multitalent_amd: cropping to the non-zero region runs on a HIP device only; there is no CPU fallback "
                       "(the host path is preprocessing/cropping.py)")


def _to_device(a, dtype=None):
    """numpy array or tensor -> contiguous device tensor (uploaded when it is not there yet); `dtype` is required, not converted to."""
    if torch.is_tensor(a):
        if not a.is_cuda:
            if not torch.cuda.is_available():
                _no_device()
            a = a.cuda()
    else:
        if not torch.cuda.is_available():
            _no_device()
        a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if dtype is not None and a.dtype != dtype:
        raise TypeError("device cropping: %s expected, got %s" % (dtype, a.dtype))
    return a.contiguous()


def _filled_mask(data):
    """data: [C, D, H, W] float32 device tensor -> (uint8 mask [D, H, W] with the holes filled, int32 device tensor [7]: box + count)."""
    assert data.dim() == 4, "data must have shape (C, X, Y, Z)"
    ops.crop_check_shape(data.shape[1:])
    with torch.cuda.device(data.device):
        return ops.fill_holes3d(ops.nonzero_mask(data))


def create_nonzero_mask(data):
    """cropping.py:23-29 -> bool device tensor [D, H, W]."""
    assert len(data.shape) == 4, "data must have shape (C, X, Y, Z)"
    return _filled_mask(_to_device(data, torch.float32))[0].view(torch.bool)


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes(mask) for a 3-D volume with the default structure -> bool device tensor; `mask` is left as it is."""
    ops.crop_check_shape(mask.shape)
    m = _to_device(mask)
    with torch.cuda.device(m.device):
        return ops.fill_holes3d((m != 0).to(torch.uint8))[0].view(torch.bool)


def get_bbox_from_mask(mask, outside_value=0):
    """cropping.py:32-40 -> [[lo, hi], ...] of Python ints, hi exclusive; an empty mask raises ValueError like np.min of nothing."""
    m = _to_device(mask) != outside_value
    bbox = []
    for a in range(m.dim()):
        along = m.any(dim=tuple(i for i in range(m.dim()) if i != a)) if m.dim() > 1 else m
        idx = torch.nonzero(along).flatten()
        if idx.numel() == 0:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        bbox.append([int(idx[0]), int(idx[-1]) + 1])
    return bbox


def crop_to_bbox(image, bbox):
    return _to_device(image)[tuple(slice(b[0], b[1]) for b in bbox)]


def crop_to_nonzero(data, seg=None, nonzero_label=-1):
    """cropping.py:84-116 -> (data, seg, bbox): device tensors of the box (data float32 bit for bit; seg int64 without a given seg,
    float32 with one, as on the host path) and the box as [[lo, hi]] * 3 of Python ints.  An all-zero volume raises ValueError."""
    data = _to_device(data, torch.float32)
    seg = _to_device(seg, torch.float32) if seg is not None else None
    mask, box = _filled_mask(data)
    b = [int(i) for i in box.cpu()]                       # the one read-back of the case
    if b[6] == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")     # the host's np.min of nothing
    with torch.cuda.device(data.device):
        out, seg_out = ops.crop_nonzero(data, mask, b[:6], seg, nonzero_label)
    if seg is None:
        seg_out = seg_out.to(torch.int64)                 # the host's mask.astype(int)
    return out, seg_out, [[b[0], b[1]], [b[2], b[3]], [b[4], b[5]]]


def get_patient_identifiers_from_cropped_files(folder):
    """cropping.py:119-120: the names of the `.npz` files of a folder without their suffix, sorted."""
    return sorted(f[:-4] for f in os.listdir(folder) if f.endswith(".npz") and os.path.isfile(os.path.join(folder, f)))


class ImageCropper(object):
    def __init__(self, num_threads, output_folder=None):
        """num_threads: host threads that read the image files and compress / write the results; output_folder: where the cropped
        cases go (created when given)."""
        self.output_folder = output_folder
        self.num_threads = num_threads
        if self.output_folder is not None:
            os.makedirs(self.output_folder, exist_ok=True)

    @staticmethod
    def crop(data, properties, seg=None):
        data, seg, bbox = crop_to_nonzero(data, seg, nonzero_label=-1)                # cropping.py:139-150
        properties["crop_bbox"] = bbox
        # np.unique(seg), int64 or (with a seg file) float32: the device reduces the volume to its distinct BIT PATTERNS, numpy
        # applies its own rules for -0.0 and NaN to those few values
        u = torch.unique(seg.view(torch.int32) if seg.dtype == torch.float32 else seg).cpu().numpy()
        properties['classes'] = np.unique(u.view(np.float32) if seg.dtype == torch.float32 else u)
        seg.masked_fill_(seg < -1, 0)
        properties["size_after_cropping"] = tuple(int(i) for i in data[0].shape)
        return data, seg, properties

    @staticmethod
    def crop_from_list_of_files(data_files, seg_file=None):
        data, seg, properties = load_case_from_list_of_files(data_files, seg_file)
        return ImageCropper.crop(data, properties, seg)

    def _is_done(self, case_identifier):
        return os.path.isfile(os.path.join(self.output_folder, "%s.npz" % case_identifier)) \
            and os.path.isfile(os.path.join(self.output_folder, "%s.pkl" % case_identifier))

    @staticmethod
    def _crop_loaded(data, seg, properties, case_identifier):
        """`crop` for the offline cropper: the same steps, with `properties['classes']` from `mt_label_presence` instead of a sort of
        the volume.  -> all_data = vstack((data, seg)) as a device tensor of numpy's result type (float32 data over an int64
        mask is float64 there), properties."""
        data, seg, bbox = crop_to_nonzero(data, seg, nonzero_label=-1)
        properties["crop_bbox"] = bbox
        as_float = seg.dtype == torch.float32
        with torch.cuda.device(seg.device):
            labels = ops.label_presence(seg if as_float else seg.float(), "the segmentation of case %s" % case_identifier)
        properties['classes'] = np.array(labels, dtype=np.float32 if as_float else np.int64)          # np.unique(seg)
        properties["size_after_cropping"] = tuple(int(i) for i in data[0].shape)
        as_numpy = {torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64, torch.int32: np.int32,
                    torch.int16: np.int16, torch.uint8: np.uint8, torch.float16: np.float16}
        both = np.result_type(as_numpy[data.dtype], as_numpy[seg.dtype])              # what np.vstack makes of the two
        to = {v: k for k, v in as_numpy.items()}[both.type]
        return torch.cat((data.to(to), seg.to(to)), 0), properties

    def _save(self, case_identifier, all_data, properties):
        """all_data: the device tensor (compressed on the device, utilities.npz_io), the members `encode_npz_device` made of it
        (only the file is written here), or a host array (numpy's writer, as before)."""
        from ..utilities import npz_io
        fname = os.path.join(self.output_folder, "%s.npz" % case_identifier)
        if isinstance(all_data, list):
            npz_io.write_npz_members(fname, all_data)
        elif torch.is_tensor(all_data) and all_data.is_cuda:
            npz_io.save_npz_device(fname, data=all_data)
        else:
            np.savez_compressed(fname, data=all_data)
        self.save_properties(case_identifier, properties)

    def load_crop_save(self, case, case_identifier, overwrite_existing=False):
        """cropping.py:152-170: `case` = the modality files and, last, the segmentation file (or None)."""
        if not torch.cuda.is_available():
            _no_device()
        print(case_identifier)
        if overwrite_existing or not self._is_done(case_identifier):
            data, seg, properties = load_case_from_list_of_files(case[:-1], case[-1])
            self._save(case_identifier, *self._crop_loaded(data, seg, properties, case_identifier))

    def get_list_of_cropped_files(self):
        return [os.path.join(self.output_folder, i + ".npz") for i in get_patient_identifiers_from_cropped_files(self.output_folder)]

    def get_patient_identifiers_from_cropped_files(self):
        return [i.split("/")[-1][:-4] for i in self.get_list_of_cropped_files()]

    def run_cropping(self, list_of_files, overwrite_existing=False, output_folder=None):
        """cropping.py:178-206: list_of_files = [[modality files ..., segmentation file or None], ...].  The ground-truth
        segmentations are copied to `gt_segmentations/`; a case whose `.npz` and `.pkl` exist is skipped unless
        `overwrite_existing`.  The cases go through the one device in sequence; host threads read ahead and write behind."""
        if not torch.cuda.is_available():
            _no_device()
        if output_folder is not None:
            self.output_folder = output_folder
        output_folder_gt = os.path.join(self.output_folder, "gt_segmentations")
        os.makedirs(output_folder_gt, exist_ok=True)
        for case in list_of_files:
            if case[-1] is not None:
                shutil.copy(case[-1], output_folder_gt)
        todo = [(case, get_case_identifier(case)) for case in list_of_files]
        todo = [(case, ident) for case, ident in todo if overwrite_existing or not self._is_done(ident)]
        threads = max(1, int(self.num_threads))
        with ThreadPoolExecutor(max_workers=threads) as pool:
            reads = [pool.submit(load_case_from_list_of_files, case[:-1], case[-1]) for case, _ in todo[:threads]]
            writes = []
            for i, (case, ident) in enumerate(todo):
                print(ident)
                try:
                    data, seg, properties = reads.pop(0).result()
                    if i + threads < len(todo):                                   # keeps `threads` reads in flight
                        nxt = todo[i + threads][0]
                        reads.append(pool.submit(load_case_from_list_of_files, nxt[:-1], nxt[-1]))
                    all_data, properties = self._crop_loaded(data, seg, properties, ident)
                    all_data = encode_npz_device(data=all_data)                   # on this thread; the pool only writes the file
                except Exception as e:
                    print("Exception in", ident, ":")
                    print(e)
                    raise e
                writes.append(pool.submit(self._save, ident, all_data, properties))
                while len(writes) > 2 * threads:                                  # bounds the volumes waiting in host memory
                    writes.pop(0).result()
            for w in writes:
                w.result()

    def load_properties(self, case_identifier):
        with open(os.path.join(self.output_folder, "%s.pkl" % case_identifier), 'rb') as f:
            return pickle.load(f)

    def save_properties(self, case_identifier, properties):
        with open(os.path.join(self.output_folder, "%s.pkl" % case_identifier), 'wb') as f:
            pickle.dump(properties, f)
