"""Timing of the crop to the non-zero region on the device against the host path (`preprocessing/cropping.py`, scipy).

Seeded float32 CT-like volumes: an elliptic body of non-zero intensities with 2 % zero voxels inside it and zeros outside —
180 x 512 x 512 (`ct180`), 512^3 (`cube512`) — and the first with a table-like slab under the body that runs into four faces of
the volume (`ct180_table`).  Per volume:
  * `device_cropping.crop_to_nonzero` on a device tensor: device events, median of --reps after a warm-up, the read-back of the
    seven box integers included;
  * the same with the upload of the uncropped volume from host memory inside the timed region;
  * its three stages on their own (mask, hole filling, crop kernel) and, for comparison, the crop step done with torch slicing
    (`data[:, box].contiguous()` plus the mask slice mapped to the -1 / 0 seg);
  * `cropping.crop_to_nonzero` on the host, same machine, one run;
  * the algorithmic bytes and the HBM-bound time from them.
Both legs must give identical data (bit patterns), seg and box, or the tool exits 1.  One JSON line per volume, all of them written
to --out.

Run: python tools/bench_cropping.py [--volumes ct180,ct180_table,cube512] [--reps 5] [--no-host] [--out FILE]
Kernel statistics: rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_cropping.py --no-host --reps 3 --volumes cube512"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy on MI355X (MI355X_MICROARCH: HBM3E peak BW row)
# per voxel of the uncropped volume: mask (4 B per channel read, 1 B written); hole filling = local (mask 1 B read, labels 4 B
# written), merge (brick faces: a quarter of the voxels, two 4 B reads), flatten (labels read + written), marks (faces only, not
# counted), fill (labels 4 B read, mask 1 B written).  Per voxel of the box: data 4 B per channel read and written, mask 1 B read,
# int8 seg 1 B written, then its widening to the host path's int64 (1 B read, 8 B written).
BYTES_PER_VOXEL = {'mask': 5, 'local': 5, 'merge': 2, 'flatten': 8, 'fill': 5}
BYTES_PER_BOX_VOXEL = {'crop': 10, 'seg_to_int64': 9}
SHAPES = {'ct180': (180, 512, 512), 'ct180_table': (180, 512, 512), 'cube512': (512, 512, 512)}


def make_volume(name, seed=0):
    rng = np.random.default_rng(seed)
    D, H, W = SHAPES[name]
    vol = np.empty((D, H, W), np.float32)
    y, x = np.ogrid[:H, :W]
    for d in range(D):                                            # slice by slice: no float64 copy of the whole volume
        r = 1.0 - ((d - 0.5 * D) / (0.45 * D)) ** 2
        s = (rng.standard_normal((H, W), dtype=np.float32) * 300 + 40)
        s[s == 0] = 1.0
        s[rng.random((H, W), dtype=np.float32) < 0.02] = 0
        s[((y - 0.48 * H) / (0.36 * H)) ** 2 + ((x - 0.5 * W) / (0.43 * W)) ** 2 > r] = 0
        vol[d] = s
    if name == 'ct180_table':
        vol[:, int(0.9 * H):int(0.9 * H) + 12, :] = 150.0           # the table: through both d faces and both w faces
        vol[:, int(0.9 * H) + 3:int(0.9 * H) + 9, 8:-8] = 0         # hollow, open at d = 0 and d = D - 1
    return vol[None]


def timed(fn, reps, torch):
    out, times = None, []
    for it in range(reps + 1):                                    # the first call is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            times.append(e0.elapsed_time(e1))
    return out, float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--volumes', default='ct180,ct180_table,cube512')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from multitalent_amd import ops
    from multitalent_amd.preprocessing import cropping, device_cropping
    lines, ok = [], True
    for name in a.volumes.split(','):
        vol = make_volume(name)
        V = int(np.prod(vol.shape[1:]))
        dev = torch.from_numpy(vol).cuda()
        (d, s, bbox), ms, ms_min = timed(lambda: device_cropping.crop_to_nonzero(dev), a.reps, torch)
        _, ms_up, _ = timed(lambda: device_cropping.crop_to_nonzero(torch.from_numpy(vol).cuda()), a.reps, torch)
        # the stages
        mask, ms_mask, _ = timed(lambda: ops.nonzero_mask(dev), a.reps, torch)
        ws = torch.empty(ops.fill_holes3d_workspace(mask.shape), dtype=torch.uint8, device='cuda')
        raw = mask.clone()
        work = torch.empty_like(mask)

        def fill():
            work.copy_(raw)
            return ops.fill_holes3d(work, ws=ws)
        _, ms_copy, _ = timed(lambda: work.copy_(raw), a.reps, torch)
        (filled, box), ms_fill, _ = timed(fill, a.reps, torch)
        b = [int(i) for i in box.cpu()]
        _, ms_crop, _ = timed(lambda: ops.crop_nonzero(dev, filled, b[:6]), a.reps, torch)
        sl = (slice(b[0], b[1]), slice(b[2], b[3]), slice(b[4], b[5]))

        def sliced():
            return dev[(slice(None),) + sl].contiguous(), (filled[sl].to(torch.int8) - 1)[None]
        (sd, ss), ms_slice, _ = timed(sliced, a.reps, torch)
        assert torch.equal(sd.view(torch.int32), d.view(torch.int32)) and torch.equal(ss.to(torch.int64), s)
        Vb = int(np.prod(d.shape[1:]))
        nbytes = sum(BYTES_PER_VOXEL.values()) * V + sum(BYTES_PER_BOX_VOXEL.values()) * Vb
        bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
        res = {'metric': 'crop_to_nonzero %s %s float32' % (name, 'x'.join(str(i) for i in vol.shape[1:])),
               'device_ms_median': ms, 'device_ms_min': ms_min, 'device_with_upload_ms_median': ms_up, 'reps': a.reps,
               'stage_ms': {'nonzero_mask': ms_mask, 'fill_holes3d': ms_fill - ms_copy, 'crop_nonzero': ms_crop,
                            'crop_with_torch_slicing': ms_slice},
               'bbox': bbox, 'filled_voxels': b[6], 'holes_filled': int(b[6] - int(raw.sum())),
               'algorithmic_bytes': nbytes, 'bytes_per_voxel': BYTES_PER_VOXEL, 'bytes_per_box_voxel': BYTES_PER_BOX_VOXEL,
               'hbm_bound_ms': bound_ms, 'share_of_hbm_bound': bound_ms / ms}
        if not a.no_host:
            t0 = time.perf_counter()
            hd, hs, hb = cropping.crop_to_nonzero(vol)
            res['host_s'] = time.perf_counter() - t0
            res['host_over_device'] = res['host_s'] * 1e3 / ms
            same = (hb == bbox and hs.dtype == np.int64 and np.array_equal(hs, s.cpu().numpy())
                    and np.array_equal(np.ascontiguousarray(hd).view(np.int32), d.cpu().numpy().view(np.int32)))
            res['identical'] = bool(same)
            ok = ok and same
            del hd, hs
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del dev, d, s, mask, raw, work, filled, ws, sd, ss, vol
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
