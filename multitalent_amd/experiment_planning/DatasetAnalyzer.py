"""`DatasetAnalyzer` (reference experiment_planning/DatasetAnalyzer.py:27-268): the dataset fingerprint of a folder of cropped cases,
with the reference's names, files and return values.  The host reads each `<case>.npz` ONCE (the reference reads it once per
modality) on `num_processes` prefetching threads and uploads it; everything per voxel runs on the device:

  foreground samples    `mt_fg_sample_count` / `mt_fg_sample_gather`: `modality[seg > 0][::10]` of all modalities of a case in one
                        pass, written into that case's slot of one [modalities, capacity] device buffer that grows geometrically;
  order statistics      `mt_select_kth_f32`: one call per slice with the 8 ranks {0, n - 1, the two neighbours of the median, of the
                        0.5 and of the 99.5 percentile};
  mean, sd              `mt_masked_moments` in double, rounded once;
  np.unique(seg)        `mt_label_presence`.

The host combines the neighbours with `_interpolate`, numpy's own float32 arithmetic for `percentile(method='linear')` and `median`.
There is no CPU path for the voxel work: without a HIP device the class raises.  The reference's `_load_seg_analyze_classes`,
`_check_if_all_in_one_region` and `_collect_class_and_region_sizes` are not called by `analyze_dataset` and are not restated."""
import json
import os
import pickle
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import ops
from ..preprocessing.device_cropping import get_patient_identifiers_from_cropped_files

default_num_threads = 8
FOREGROUND_STRIDE = 10                       # `modality[mask][::10]`, DatasetAnalyzer.py:167
STAT_KEYS = ('median', 'mean', 'sd', 'mn', 'mx', 'percentile_99_5', 'percentile_00_5')


def _no_device():
    raise RuntimeError("multitalent_amd: the dataset analysis runs on a HIP device only; there is no CPU fallback")


def _virtual_index(n, q):
    """numpy's `(n - 1) * quantile` of `percentile(float32 array, q)`: the quantile is q / float32(100) and the index is formed in
    float32 too.  -> (previous index, next index, gamma as np.float32); both indices are the last one at or beyond n - 1."""
    quantile = np.true_divide(q, np.float32(100))
    vi = np.float32((n - 1) * quantile)
    if not vi < n - 1:
        return n - 1, n - 1, np.float32(0)
    prev = int(np.floor(vi))
    prev = min(max(prev, 0), n - 1)
    return prev, min(prev + 1, n - 1), np.float32(vi - np.float32(prev))


def _neighbour_ranks(n, q):
    """The two 0-based ranks of the sorted sample that `_interpolate(lo, hi, n, q)` combines; q: a percentage or 'median'."""
    if q == 'median':
        return (n - 1) // 2, n // 2
    return _virtual_index(n, q)[:2]


def _interpolate(lo_value, hi_value, n, q):
    """numpy's `np.percentile(x, q)` (method 'linear') or, with q = 'median', `np.median(x)` of n float32 samples, from the two order
    statistics at `_neighbour_ranks(n, q)`, in numpy's float32 operations and their order -> np.float32."""
    a, b = np.float32(lo_value), np.float32(hi_value)
    with np.errstate(all='ignore'):
        if q == 'median':
            return a if n % 2 == 1 else np.float32(np.float32(a + b) / np.float32(2))
        t = _virtual_index(n, q)[2]
        d = np.float32(b - a)
        if t >= 0.5:
            return np.float32(b - np.float32(d * np.float32(np.float32(1) - t)))
        return np.float32(a + np.float32(d * t))


def _stat_ranks(n):
    """The eight ranks of one select call: mn, mx, and the neighbours of the median, the 99.5 and the 0.5 percentile."""
    return [0, n - 1, *_neighbour_ranks(n, 'median'), *_neighbour_ranks(n, 99.5), *_neighbour_ranks(n, 0.5)]


def _combine(n, order, moments, nans):
    """order: the 8 float32 order statistics of `_stat_ranks(n)`, moments: (count, mean, sd) in double, nans: NaNs among the samples
    -> the seven values of `_compute_stats` in the reference's order."""
    if n == 0:
        return (np.nan,) * 7
    if nans:
        return (np.float32(np.nan),) * 7
    o = [np.float32(v) for v in order]
    return (_interpolate(o[2], o[3], n, 'median'), np.float32(moments[1]), np.float32(moments[2]), o[0], o[1],
            _interpolate(o[4], o[5], n, 99.5), _interpolate(o[6], o[7], n, 0.5))


class _Pending:
    """Device results of one slice of samples, read back together at the end."""

    def __init__(self, n, order=None, moments=None, nans=None):
        self.n, self.order, self.moments, self.nans = n, order, moments, nans


def _launch_stats(x):
    """x: 1-D float32 device tensor (a view is fine) -> (order statistics [8], moments [1, 3]) on the device, nothing synchronised."""
    n = int(x.numel())
    return ops.select_kth_f32(x, _stat_ranks(n)), ops.masked_moments(x[None], ops.MOMENTS_ALL)


class DatasetAnalyzer(object):
    def __init__(self, folder_with_cropped_data, overwrite=True, num_processes=default_num_threads):
        """overwrite=False loads the pickles of an earlier run where they exist.  num_processes: host threads that read and
        decompress the `.npz` files ahead of the device."""
        self.num_processes = num_processes
        self.overwrite = overwrite
        self.folder_with_cropped_data = folder_with_cropped_data
        self.sizes = self.spacings = None
        self.patient_identifiers = get_patient_identifiers_from_cropped_files(self.folder_with_cropped_data)
        assert os.path.isfile(os.path.join(self.folder_with_cropped_data, "dataset.json")), \
            "dataset.json needs to be in folder_with_cropped_data"
        self.props_per_case_file = os.path.join(self.folder_with_cropped_data, "props_per_case.pkl")
        self.intensityproperties_file = os.path.join(self.folder_with_cropped_data, "intensityproperties.pkl")

    def load_properties_of_cropped(self, case_identifier):
        with open(os.path.join(self.folder_with_cropped_data, "%s.pkl" % case_identifier), 'rb') as f:
            return pickle.load(f)

    def _load_json(self):
        with open(os.path.join(self.folder_with_cropped_data, "dataset.json"), 'r') as f:
            return json.load(f)

    def get_classes(self):
        return self._load_json()['labels']

    def get_modalities(self):
        modalities = self._load_json()["modality"]
        return {int(k): modalities[k] for k in modalities.keys()}

    def _load_case(self, patient_identifier):
        return np.load(os.path.join(self.folder_with_cropped_data, patient_identifier) + ".npz")['data']

    def _load_case_device(self, patient_identifier, device=None):
        """the cropped case [C + 1, X, Y, Z] as a device tensor: its compressed bytes are uploaded and inflated there
        (utilities.npz_io.load_npz_device); a file of another writer is read by `np.load` inside the reader.
        device None: the calling thread's current device."""
        from ..utilities.npz_io import load_npz_device
        fname = os.path.join(self.folder_with_cropped_data, patient_identifier) + ".npz"
        return load_npz_device(fname, 'data', torch.device('cuda', torch.cuda.current_device()) if device is None else device)

    @staticmethod
    def _float32_on_device(a, dev='cuda'):
        if torch.is_tensor(a):
            return a.to(device=dev, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

    def _prefetched_cases(self):
        """(identifier, array) in order; up to num_processes files are read (and inflated, on the device) ahead from host threads."""
        ahead = max(1, int(self.num_processes))
        dev = torch.device('cuda', torch.cuda.current_device())          # the caller's device (the current one is per thread)
        with ThreadPoolExecutor(max_workers=ahead) as pool:
            pending = []
            ids = iter(self.patient_identifiers)
            for p in ids:
                pending.append((p, pool.submit(self._load_case_device, p, dev)))
                if len(pending) >= ahead:
                    break
            while pending:
                p, fut = pending.pop(0)
                nxt = next(ids, None)
                if nxt is not None:
                    pending.append((nxt, pool.submit(self._load_case_device, nxt, dev)))
                yield p, fut.result()

    def analyse_segmentations(self):
        class_dct = self.get_classes()
        if self.overwrite or not os.path.isfile(self.props_per_case_file):
            if not torch.cuda.is_available():
                _no_device()
            props_per_patient = OrderedDict()
            for p, all_data in self._prefetched_cases():
                seg = self._float32_on_device(all_data[-1])
                labels = ops.label_presence(seg, "the segmentation of case %s" % p)
                dtype = np.dtype(str(all_data.dtype).replace('torch.', ''))
                props_per_patient[p] = {'has_classes': np.array(labels, dtype=dtype)}       # np.unique(seg)
            with open(self.props_per_case_file, 'wb') as f:
                pickle.dump(props_per_patient, f)
        else:
            with open(self.props_per_case_file, 'rb') as f:
                props_per_patient = pickle.load(f)
        return class_dct, props_per_patient

    def get_sizes_and_spacings_after_cropping(self):
        sizes, spacings = [], []
        for c in self.patient_identifiers:
            properties = self.load_properties_of_cropped(c)
            sizes.append(properties["size_after_cropping"])
            spacings.append(properties["original_spacing"])
        return sizes, spacings

    def get_size_reduction_by_cropping(self):
        size_reduction = OrderedDict()
        for p in self.patient_identifiers:
            props = self.load_properties_of_cropped(p)
            size_reduction[p] = np.prod(props['size_after_cropping']) / np.prod(props["original_size_of_raw_data"])
        return size_reduction

    @staticmethod
    def _compute_stats(voxels):
        """voxels: a 1-D float32 tensor (device or host) or array -> median, mean, sd, mn, mx, percentile_99_5, percentile_00_5."""
        if not torch.cuda.is_available():
            _no_device()
        if not torch.is_tensor(voxels):
            voxels = torch.from_numpy(np.ascontiguousarray(np.asarray(voxels, dtype=np.float32).reshape(-1)))
        x = voxels.reshape(-1).to(device='cuda', dtype=torch.float32).contiguous()
        n = int(x.numel())
        if n == 0:
            return _combine(0, None, None, 0)
        with torch.cuda.device(x.device):
            order, moments = _launch_stats(x)
            nans = int(torch.isnan(x).sum().item())
        return _combine(n, order.cpu().numpy(), moments.cpu().numpy()[0], nans)

    def collect_intensity_properties(self, num_modalities):
        if self.overwrite or not os.path.isfile(self.intensityproperties_file):
            if not torch.cuda.is_available():
                _no_device()
            results = self._assemble(int(num_modalities), *self._device_statistics(int(num_modalities)))
            with open(self.intensityproperties_file, 'wb') as f:
                pickle.dump(results, f)
        else:
            with open(self.intensityproperties_file, 'rb') as f:
                results = pickle.load(f)
        return results

    def _device_statistics(self, M):
        """-> (local, glob, nans): local[c][i] / glob[c] the `_Pending` of modality c for case i / for all samples, with its order
        statistics and moments on the host; nans[i, c] the NaNs among the samples of case i."""
        dev = torch.device('cuda', torch.cuda.current_device())
        buf = torch.empty((M, 1 << 16), dtype=torch.float32, device=dev) if M > 0 else None
        total = 0
        local = [[] for _ in range(M)]                         # per modality: one _Pending per case
        case_nans = []
        for p, all_data in self._prefetched_cases():
            if M == 0:
                continue
            if all_data.shape[0] < M + 1:
                raise ValueError("case %s holds %d modalities, %d expected" % (p, all_data.shape[0] - 1, M))
            vol = self._float32_on_device(all_data, dev)
            vol = vol.reshape(vol.shape[0], -1)
            data, seg = vol[:M], vol[-1]
            index = ops.fg_sample_count(seg)
            m = (index.n + FOREGROUND_STRIDE - 1) // FOREGROUND_STRIDE          # the count reaches the host once per case
            if total + m > buf.shape[1]:
                grown = torch.empty((M, max(2 * buf.shape[1], total + m)), dtype=torch.float32, device=dev)
                grown[:, :total] = buf[:, :total]
                buf = grown
            samples, n, nans = ops.fg_sample(data, seg, FOREGROUND_STRIDE, out=buf, offset=total, index=index)
            case_nans.append(nans)
            for c in range(M):
                local[c].append(_Pending(m, *(_launch_stats(samples[c]) if m > 0 else (None, None))))
            total += m
        glob = [_Pending(total, *(_launch_stats(buf[c, :total]) if total > 0 else (None, None))) for c in range(M)]
        # one read-back of everything
        nan_host = torch.stack(case_nans).cpu().numpy() if case_nans else np.zeros((0, M), dtype=np.int64)
        live = [q for c in range(M) for q in local[c] + [glob[c]] if q.n > 0]
        if live:
            order = torch.stack([q.order for q in live]).cpu().numpy()
            moments = torch.stack([q.moments[0] for q in live]).cpu().numpy()
            for i, q in enumerate(live):
                q.order, q.moments = order[i], moments[i]
        return local, glob, nan_host

    def _assemble(self, M, local, glob, nan_host):
        """The reference's nested OrderedDicts (DatasetAnalyzer.py:199-217) from the statistics of `_device_statistics`."""
        results = OrderedDict()
        for c in range(M):
            results[c] = OrderedDict()
            props_per_case = OrderedDict()
            for i, pat in enumerate(self.patient_identifiers):
                q = local[c][i]
                props_per_case[pat] = OrderedDict(zip(STAT_KEYS, _combine(q.n, q.order, q.moments, int(nan_host[i, c]))))
            results[c]['local_props'] = props_per_case
            g = glob[c]
            for k, v in zip(STAT_KEYS, _combine(g.n, g.order, g.moments, int(nan_host[:, c].sum()) if len(nan_host) else 0)):
                results[c][k] = v
        return results

    def analyze_dataset(self, collect_intensityproperties=True):
        sizes, spacings = self.get_sizes_and_spacings_after_cropping()
        classes = self.get_classes()
        all_classes = [int(i) for i in classes.keys() if int(i) > 0]
        modalities = self.get_modalities()
        if collect_intensityproperties:
            intensityproperties = self.collect_intensity_properties(len(modalities))
        else:
            intensityproperties = None
        size_reductions = self.get_size_reduction_by_cropping()
        dataset_properties = dict()
        dataset_properties['all_sizes'] = sizes
        dataset_properties['all_spacings'] = spacings
        dataset_properties['all_classes'] = all_classes
        dataset_properties['modalities'] = modalities
        dataset_properties['intensityproperties'] = intensityproperties
        dataset_properties['size_reductions'] = size_reductions
        with open(os.path.join(self.folder_with_cropped_data, "dataset_properties.pkl"), 'wb') as f:
            pickle.dump(dataset_properties, f)
        return dataset_properties
