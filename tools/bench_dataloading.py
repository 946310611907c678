"""Batches per second of the training loaders, and the bandwidth of the patch gather.

Seeded synthetic preprocessed cases, 180 x 512 x 512, one modality, written to a temporary folder as .npz + unpacked .npy (what
`run_training` reads).  Two configurations: B = 2 at the loader patch of the 48 x 192 x 192 network patch (161 x 308 x 225) and B = 4 at
the loader patch of Task100's native 96 x 192 x 192 patch, oversampling 0.33, constant padding.  For each, --batches batches after a
warm-up, a host clock around work that ends in a device synchronise:
  * host      `DataLoader3D` and the upload `MoreDADeviceAugmenter` does with a host batch (pageable memory): the path before the
              device loader, the baseline;
  * resident  `DeviceDataLoader3D` with every case resident (the warm-up uploads them);
  * staged    `DeviceDataLoader3D` with a budget of 0: every sample's valid sub-box goes through pinned memory.
The three draw the same batches from the same seed; the tool checks the first batch of each against the host's, bit for bit.
Then `mt_patch_gather` alone on resident cases (device events, median of --reps): its time, the minimum traffic of
(4C + 2) bytes read and 4(C + 1) written per patch voxel, and the bandwidth that gives, to be read against the float4 streaming
figure of DESIGN.md.  With --peak: `torch.cuda.max_memory_allocated()` after training steps of the Task100 residual encoder and
of the Task100 network (bench.py's synthetic batch), the number `device_case_cache_fraction` is sized against.
One JSON line per measurement, all of them written to --out.

Run: python tools/bench_dataloading.py [--cases 4] [--batches 8] [--reps 5] [--peak] [--out FILE]"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

SHAPE = (180, 512, 512)
NETWORK_PATCHES = {'patch48': ((48, 192, 192), 2), 'task100_native': ((96, 192, 192), 4)}


def write_cases(folder, n, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(SHAPE, dtype=np.float32)
    for k in range(n):
        seg = np.zeros(SHAPE, np.float32)
        for lab in (1, 2, 3):
            sz = [int(s * rng.uniform(0.15, 0.4)) for s in SHAPE]
            lo = [int(rng.integers(0, s - z + 1)) for s, z in zip(SHAPE, sz)]
            seg[lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = lab
        seg[:, :9, :] = -1
        arr = np.stack([base + np.float32(k), seg])
        name = 'CT_%02d' % k
        np.savez(os.path.join(folder, name + '.npz'), data=arr)          # stored, not deflated: only the .npy is read
        np.save(os.path.join(folder, name + '.npy'), arr)
        locs = {}
        for lab in (1, 2, 3):
            al = np.argwhere(seg == lab)
            locs[lab] = al[rng.choice(len(al), min(10000, len(al)), replace=False)] if len(al) else al
        with open(os.path.join(folder, name + '.pkl'), 'wb') as f:
            pickle.dump({'class_locations': locs}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', type=int, default=4)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--peak', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dataloading needs a HIP device: a host run measures nothing")
    from multitalent_amd import ops
    from multitalent_amd.training.data_augmentation.color import default_3d_augmentation_params
    from multitalent_amd.training.data_augmentation.spatial import get_patch_size
    from multitalent_amd.training.dataloading import dataset_loading as dl
    from multitalent_amd.training.dataloading.device_loading import DeviceCaseCache, DeviceDataLoader3D
    dev = torch.device('cuda', torch.cuda.current_device())
    lines = []

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    p = default_3d_augmentation_params()
    with tempfile.TemporaryDirectory() as folder:
        write_cases(folder, a.cases)
        ds = dl.load_dataset(folder)
        for name, (net_patch, B) in NETWORK_PATCHES.items():
            ps = tuple(int(i) for i in get_patch_size(net_patch, p['rotation_x'], p['rotation_y'], p['rotation_z'], (0.85, 1.25)))
            kw = dict(oversample_foreground_percent=0.33, pad_mode='constant', memmap_mode='r')

            def host_batch(loader):
                b = next(loader)
                return (torch.from_numpy(b['data']).to(dev, non_blocking=True), torch.from_numpy(b['seg'][:, :1]).to(dev, non_blocking=True))

            def device_batch(loader):
                b = next(loader)
                return b['data'], b['seg']

            resident = DeviceCaseCache(dev, 1 << 40)
            paths = [('host', lambda: dl.DataLoader3D(ds, ps, net_patch, B, False, **kw), host_batch),
                     ('resident', lambda: DeviceDataLoader3D(ds, ps, net_patch, B, False, cache=resident, **kw), device_batch),
                     ('staged', lambda: DeviceDataLoader3D(ds, ps, net_patch, B, False, cache=DeviceCaseCache(dev, 0), **kw), device_batch)]
            first, rate = {}, {}
            for path, make, draw in paths:
                np.random.seed(0)
                loader = make()
                first[path] = tuple(t.cpu().numpy() for t in draw(loader))
                for _ in range(a.cases * 2 if path == 'resident' else 1):         # warm-up: code objects, pinned buffers, residency
                    draw(loader)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.batches):
                    out = draw(loader)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                del out
                rate[path] = a.batches / dt
                emit({'metric': 'loader batches/s, %s, B=%d, loader patch %s, cases %s C=1' % (path, B, 'x'.join(map(str, ps)), 'x'.join(map(str, SHAPE))),
                      'config': name, 'path': path, 'batches_per_s': rate[path], 'patches_per_s': rate[path] * B, 'ms_per_batch': dt / a.batches * 1e3,
                      'batches': a.batches, 'resident_cases': len(resident) if path == 'resident' else 0,
                      'identical_to_host_first_batch': all(np.array_equal(x, y) for x, y in zip(first[path], first['host']))})
            emit({'metric': 'loader speed-up over the host loader + upload', 'config': name,
                  'resident_over_host': rate['resident'] / rate['host'], 'staged_over_host': rate['staged'] / rate['host']})
            # the kernel alone
            cases = [resident.get(f) for f in resident.resident_files()]
            rng = np.random.default_rng(1)
            sources = []
            for j in range(B):
                c = cases[j % len(cases)]
                sources.append((c.data, c.seg, [int(rng.integers(min(0, s - q), max(0, s - q) + 1)) for s, q in zip(c.shape, ps)]))
            data_out, seg_out = ops.patch_gather(sources, ps, 'constant')
            times = []
            for it in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.patch_gather(sources, ps, 'constant', data_out, seg_out)
                e1.record()
                torch.cuda.synchronize()
                if it:
                    times.append(e0.elapsed_time(e1))
            ms = float(np.median(times))
            pv = B * int(np.prod(ps))
            nbytes = pv * ((4 * 1 + 2) + 4 * (1 + 1))
            emit({'metric': 'mt_patch_gather, B=%d, C=1, patch %s' % (B, 'x'.join(map(str, ps))), 'config': name, 'kernel_ms_median': ms, 'reps': a.reps,
                  'min_bytes': nbytes, 'gb_per_s_of_min_traffic': nbytes / (ms * 1e-3) / 1e9})
            del resident, cases, sources, data_out, seg_out
            torch.cuda.empty_cache()
    if a.peak:
        import bench
        total = torch.cuda.get_device_properties(dev).total_memory
        for workload, precision, B in (('resenc', 'fp32', 4), ('resenc', 'fp32', 2), ('task100', 'fp32', 4)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            r = bench.time_training(workload, precision, bench.PATCH, B, 2, 1, dev, 0, 1, False)
            peak = torch.cuda.max_memory_allocated()
            emit({'metric': 'peak device memory of training steps (torch.cuda.max_memory_allocated)', 'workload': workload, 'precision': precision,
                  'batch': B, 'patch': list(bench.PATCH), 'peak_bytes': int(peak), 'device_total_bytes': int(total), 'peak_share_of_device': peak / total})
            del r
            bench.net_cache_clear()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
