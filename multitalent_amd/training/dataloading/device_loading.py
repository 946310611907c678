"""Training batches from cases that live on the device: `DataLoader3D` (dataset_loading.py; reference
`nnunet/training/dataloading/dataset_loading.py:224-380`) with its host memcpy replaced by one gather launch.

The host loader copies every box out of a memory-mapped file, pads it into a zeroed batch and leaves the upload of the whole
(oversized) loader patch to the augmenter, all inside the training thread.  Here

  DeviceCaseCache      keeps whole preprocessed cases on the device: the C image channels as float32, the label channel as int16
                       (`mt_seg_narrow` proves that nothing is lost), `C*V*4 + V*2` bytes a case, up to a byte budget, no eviction;
  DeviceDataLoader3D   makes the host loader's random draws in its order (`plan_batch`, host only: a seeded run draws the very
                       batches of the host loader) and fills the batch with `mt_patch_gather`: a resident sample costs a
                       descriptor in the kernel arguments; of a non-resident one only the valid sub-box of the patch is staged
                       (pinned) and uploaded.

The batches are bit-identical to the host loader's (tests/test_device_loading_gpu.py pins them to tests/golden/loader.npz).
There is no CPU gather: without a HIP device only `plan_batch` works."""
import os
from collections import namedtuple

import numpy as np
import torch

from .dataset_loading import DataLoader3D, load_pickle

ResidentCase = namedtuple('ResidentCase', 'data seg shape properties')      # data [C, x, y, z] f32, seg [x, y, z] int16: device


def _case_file_array(entry, device=None):
    """The whole [C+1, x, y, z] array of a case: the unpacked .npy when present, else the .npz (DataLoader3D._load_case) — with a
    `device`, inflated there (utilities.npz_io.load_npz_device) and returned as a device tensor."""
    f = entry['data_file']
    if os.path.isfile(f[:-4] + ".npy"):
        return np.load(f[:-4] + ".npy", 'r')
    if device is not None:
        from ...utilities.npz_io import load_npz_device
        return load_npz_device(f, 'data', device)
    return np.load(f)['data']


class DeviceCaseCache:
    """A static resident set of preprocessed cases on `device`.  The first time a case is offered and its `C*V*4 + V*2` bytes
    still fit `budget_bytes` it becomes resident for good; a case that does not fit stays on the host for the life of the cache.
    No eviction on purpose: under random sampling of a dataset larger than the budget an LRU would upload a whole case to use one
    patch of it.  `used_bytes` is exactly the sum of `case_bytes` of the residents (no rounding), so a caller can size a budget.
    The properties dict of a resident case is kept with it."""

    def __init__(self, device, budget_bytes):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("DeviceCaseCache needs a HIP device (the host loader is DataLoader3D)")
        self.budget_bytes = int(budget_bytes)
        self.used_bytes = 0
        self._cases = {}                 # data_file -> ResidentCase
        self._pinned = None              # staging buffer of the uploads, grown to the largest case seen

    @staticmethod
    def case_bytes(shape):
        """shape: [C+1, x, y, z] of a case on disk -> its bytes on the device."""
        v = int(np.prod([int(i) for i in shape[1:]], dtype=np.int64))
        return (int(shape[0]) - 1) * v * 4 + v * 2

    def __len__(self):
        return len(self._cases)

    def __contains__(self, data_file):
        return data_file in self._cases

    def resident_files(self):
        return list(self._cases)

    def get(self, data_file):
        return self._cases.get(data_file)

    def room_for(self, entry):
        """False when the case of `entry` is known not to fit what is left of the budget.  For a case that exists as .npz only the
        shape comes from the .npy header at the head of the member (utilities.npz_io.peek_npy_header: nothing else is inflated);
        where it cannot be told this way the answer is True and `admit` decides on the array."""
        if self.used_bytes >= self.budget_bytes:
            return False
        f = entry['data_file']
        if os.path.isfile(f[:-4] + ".npy") or not os.path.isfile(f):
            return True
        from ...utilities.npz_io import peek_npy_header
        head = peek_npy_header(f, 'data')
        return head is None or len(head[0]) != 4 or self.used_bytes + self.case_bytes(head[0]) <= self.budget_bytes

    def admit(self, entry, all_data=None, properties=None):
        """entry: a `load_dataset` entry.  -> its ResidentCase (uploading it now when it fits the budget), or None.
        all_data / properties: what the caller has already read of the case."""
        key = entry['data_file']
        res = self._cases.get(key)
        if res is not None:
            return res
        if all_data is None:
            if not self.room_for(entry):
                return None                  # known from the header alone: nothing is read or inflated for a case that cannot stay
            all_data = _case_file_array(entry, self.device)
        need = self.case_bytes(all_data.shape)
        if self.used_bytes + need > self.budget_bytes:
            return None
        if properties is None:
            properties = entry['properties'] if 'properties' in entry else load_pickle(entry['properties_file'])
        from ... import ops
        c, shape = all_data.shape[0] - 1, tuple(int(i) for i in all_data.shape[1:])
        v = int(np.prod(shape, dtype=np.int64))
        on_device = torch.is_tensor(all_data) and all_data.is_cuda and all_data.dtype == torch.float32
        if torch.is_tensor(all_data) and not on_device:
            all_data = all_data.float().cpu().numpy()
        if not on_device:
            if self._pinned is None or self._pinned.numel() < (c + 1) * v:
                self._pinned = None
                self._pinned = torch.empty((c + 1) * v, dtype=torch.float32).pin_memory()
            np.copyto(self._pinned.numpy()[:(c + 1) * v].reshape(all_data.shape), all_data)
        with torch.cuda.device(self.device):
            if on_device:                    # read by load_npz_device: the channels are copied out of the inflated member,
                data, segf = all_data[:c].clone(), all_data[c].clone()      # which is then free again
                del all_data
            else:
                data = torch.empty((c,) + shape, dtype=torch.float32, device=self.device)
                data.view(-1).copy_(self._pinned[:c * v], non_blocking=True)
                segf = torch.empty(shape, dtype=torch.float32, device=self.device)
                segf.view(-1).copy_(self._pinned[c * v:(c + 1) * v], non_blocking=True)
            flag = torch.zeros(1, dtype=torch.int32, device=self.device)
            seg = ops.seg_narrow(segf, flag)
            bad = int(flag.item())           # the one synchronisation of an upload: the staging buffer is free again after it
        if bad:
            raise RuntimeError("the label channel of case %s holds a value that is not an integer of int16 (a fraction, a NaN or a "
                               "label beyond +-32767): it cannot be kept as int16 on the device" % key)
        res = ResidentCase(data, seg, shape, properties)
        self._cases[key] = res
        self.used_bytes += need
        return res


class _Slot:
    """Pinned staging memory of one sample position and the event recorded behind its last upload."""

    def __init__(self):
        self.pinned, self.event = None, None

    def buffer(self, n):
        if self.event is not None:
            self.event.synchronize()         # reuse only after the upload that last read this memory has completed
            self.event = None
        if self.pinned is None or self.pinned.numel() < n:
            self.pinned = None
            self.pinned = torch.empty(n, dtype=torch.float32).pin_memory()
        return self.pinned


class DeviceDataLoader3D(DataLoader3D):
    """DataLoader3D whose batches are device tensors: {'data' [B, C, *patch] f32, 'seg' [B, 1, *patch] f32, 'properties', 'keys'}.
    Same constructor, attributes and random draws; `cache`: a DeviceCaseCache (shared between loaders), None = nothing resident.
    Padding: 'constant' (zeros) and 'edge'.  Cascade inputs (`has_prev_stage`) are out of scope in this package."""

    def __init__(self, data, patch_size, final_patch_size, batch_size, has_prev_stage=False, oversample_foreground_percent=0.0,
                 memmap_mode="r", pad_mode="edge", pad_kwargs_data=None, pad_sides=None, sampling_probabilities=None, cache=None):
        if has_prev_stage:
            raise NotImplementedError("DeviceDataLoader3D: the segmentations of a previous stage (cascade) are not supported")
        if pad_mode not in ('constant', 'edge'):
            raise NotImplementedError("DeviceDataLoader3D: pad mode %r (the gather pads with 'constant' zeros or 'edge')" % (pad_mode,))
        if pad_kwargs_data and (pad_mode != 'constant' or set(pad_kwargs_data) != {'constant_values'} or pad_kwargs_data['constant_values'] != 0):
            raise NotImplementedError("DeviceDataLoader3D: pad_kwargs_data %r (only zeros are padded)" % (dict(pad_kwargs_data),))
        super().__init__(data, patch_size, final_patch_size, batch_size, has_prev_stage, oversample_foreground_percent, memmap_mode,
                         pad_mode, pad_kwargs_data, pad_sides, sampling_probabilities)
        self.cache = cache
        self._slots = [_Slot() for _ in range(self.batch_size)]
        self._flags = None

    def determine_shapes(self):
        """as DataLoader3D's; the channel count of a first case that exists as .npz only comes from the .npy header at the head of
        the member, so that no case is inflated on the host just to be counted"""
        entry = self._data[list(self._data.keys())[0]]
        f = entry['data_file']
        if not os.path.isfile(f[:-4] + ".npy") and os.path.isfile(f):
            from ...utilities.npz_io import peek_npy_header
            head = peek_npy_header(f, 'data')
            if head is not None and len(head[0]) == 4:
                return (self.batch_size, head[0][0] - 1, *self.patch_size), (self.batch_size, 1, *self.patch_size)
        return super().determine_shapes()

    def plan_batch(self):
        """The host half of generate_train_batch (without a cache, without a device): exactly its draws from numpy's global stream, in its order (the
        keys; per sample the foreground class and voxel, or three randint).  -> {'keys', 'properties' [B], 'bb_lb' [B][3] (lower
        corner of each patch in case coordinates, may be negative), 'shapes' [B][3], 'entries' [B], 'cases' [B] (the opened array of
        a sample whose case is not resident, else None)}.  With a cache, a case that exists as .npz only and fits the budget is
        admitted here, through the device reader; the host opens (and inflates) only a case that will be staged."""
        selected_keys = np.random.choice(self.list_of_keys, self.batch_size, True, self.sampling_probabilities)
        plan = {'keys': selected_keys, 'properties': [], 'bb_lb': [], 'shapes': [], 'entries': [], 'cases': []}
        for j, i in enumerate(selected_keys):
            force_fg = self.get_do_oversample(j)
            entry = self._data[i]
            res = self.cache.get(entry['data_file']) if self.cache is not None else None
            if res is not None:
                properties, case_all_data, shape = res.properties, None, res.shape
            else:
                properties = entry['properties'] if 'properties' in entry.keys() else load_pickle(entry['properties_file'])
                if self.cache is not None and not os.path.isfile(entry['data_file'][:-4] + ".npy") and self.cache.room_for(entry):
                    # a case that exists as .npz only and still fits: it goes resident now, inflated on the device
                    # (DeviceCaseCache.admit -> utilities.npz_io.load_npz_device), and never exists uncompressed on the host
                    res = self.cache.admit(entry, None, properties)
                if res is not None:
                    case_all_data, shape = None, res.shape
                else:
                    case_all_data = self._load_case(entry)
                    shape = tuple(int(s) for s in case_all_data.shape[1:])
            need_to_pad = self.need_to_pad.copy()
            for d in range(3):
                if need_to_pad[d] + shape[d] < self.patch_size[d]:
                    need_to_pad[d] = self.patch_size[d] - shape[d]
            lb = [-need_to_pad[d] // 2 for d in range(3)]
            ub = [shape[d] + need_to_pad[d] // 2 + need_to_pad[d] % 2 - self.patch_size[d] for d in range(3)]
            voxels = None
            if force_fg:
                if 'class_locations' not in properties.keys():
                    raise RuntimeError("Please rerun the preprocessing with the newest version of nnU-Net!")
                fg = np.array([c for c in properties['class_locations'].keys() if len(properties['class_locations'][c]) != 0])
                fg = fg[fg > 0]
                if len(fg) == 0:
                    print('case does not contain any foreground classes', i)
                else:
                    voxels = properties['class_locations'][np.random.choice(fg)]
            if voxels is not None:
                sel = voxels[np.random.choice(len(voxels))]
                bb_lb = [max(lb[d], sel[d] - self.patch_size[d] // 2) for d in range(3)]
            else:
                bb_lb = [np.random.randint(lb[d], ub[d] + 1) for d in range(3)]
            plan['properties'].append(properties)
            plan['bb_lb'].append([int(b) for b in bb_lb])
            plan['shapes'].append(shape)
            plan['entries'].append(entry)
            plan['cases'].append(case_all_data)
        return plan

    def _device(self):
        if self.cache is not None:
            return self.cache.device
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceDataLoader3D needs a HIP device to fill a batch (the host loader is DataLoader3D)")
        return torch.device('cuda', torch.cuda.current_device())

    def gather(self, plan, data_out=None, seg_out=None):
        """The device half: one descriptor per sample, then `mt_patch_gather`.  -> (data, seg) device tensors (data_out / seg_out when
        given).  A sample whose case is not resident, and does not become resident now, is staged: the valid sub-box [vlb, vub) of its
        patch goes through pinned memory onto the device and the descriptor addresses the patch relative to that box, which is bit
        for bit the same in both pad modes (what lies outside the box lies outside the case, in the same direction)."""
        from ... import ops
        dev = self._device()
        ps = [int(p) for p in self.patch_size]
        sources, staged = [], []
        with torch.cuda.device(dev):
            for j, (entry, arr, bb_lb, shape) in enumerate(zip(plan['entries'], plan['cases'], plan['bb_lb'], plan['shapes'])):
                res = None
                if self.cache is not None:
                    res = self.cache.get(entry['data_file'])
                    if res is None:
                        res = self.cache.admit(entry, arr, plan['properties'][j])
                if res is not None:
                    sources.append((res.data, res.seg, bb_lb))
                    continue
                if arr is None:
                    arr = self._load_case(entry)
                vlb = [max(0, bb_lb[d]) for d in range(3)]
                vub = [min(shape[d], bb_lb[d] + ps[d]) for d in range(3)]
                box = tuple(vub[d] - vlb[d] for d in range(3))
                if min(box) < 1:
                    raise RuntimeError("DeviceDataLoader3D: the patch at %s misses case %s of shape %s" % (bb_lb, plan['keys'][j], shape))
                c, bv = arr.shape[0] - 1, box[0] * box[1] * box[2]
                n = (c + 1) * bv
                slot = self._slots[j]
                pinned = slot.buffer((c + 1) * ps[0] * ps[1] * ps[2])
                np.copyto(pinned.numpy()[:n].reshape((c + 1,) + box), arr[:, vlb[0]:vub[0], vlb[1]:vub[1], vlb[2]:vub[2]])
                buf = torch.empty(n, dtype=torch.float32, device=dev)
                buf.copy_(pinned[:n], non_blocking=True)
                slot.event = torch.cuda.Event()
                slot.event.record()
                if self._flags is None:
                    self._flags = torch.zeros(self.batch_size, dtype=torch.int32, device=dev)
                if not staged:
                    self._flags.zero_()
                seg = ops.seg_narrow(buf[c * bv:].view(box), self._flags[j:j + 1])
                sources.append((buf[:c * bv].view((c,) + box), seg, [bb_lb[d] - vlb[d] for d in range(3)]))
                staged.append(j)
            data, seg = ops.patch_gather(sources, ps, self.pad_mode, data_out, seg_out, seg_fill=-1.0)
            if staged:
                bad = self._flags.cpu().numpy()          # staged label boxes are checked as they pass: one read-back per batch
                if bad.any():
                    raise RuntimeError("the label channel of case %s holds a value that is not an integer of int16 (a fraction, a NaN "
                                       "or a label beyond +-32767)" % ', '.join(str(plan['keys'][j]) for j in staged if bad[j]))
        return data, seg

    def generate_train_batch(self, data_out=None, seg_out=None):
        plan = self.plan_batch()
        data, seg = self.gather(plan, data_out, seg_out)
        return {'data': data, 'seg': seg, 'properties': plan['properties'], 'keys': plan['keys']}
