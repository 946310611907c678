"""Timing of the connected-component postprocessing on the device against the reference's host path.

One seeded 512^3 label volume with three classes — one large organ-like blob per class, a few hundred small spurious blobs, and
a slab at the 6-connectivity site-percolation density (0.3116, the hardest case for union-find) — goes through
`remove_all_but_the_largest_connected_component(image, [1, 2, 3], vpv)` on the device (device events, after a warm-up), and
through scipy.ndimage.label plus the reference's removal loop (connected_components.py:48-101, restated here with scipy) on the
host.  Both outputs must be identical.  The algorithmic bytes of one labelling + removal pass and the HBM-bound time from them
are printed with the measured times as one JSON line (and written to --out).

Run: python tools/bench_postprocessing.py [--size 512] [--reps 5] [--no-host] [--out FILE]
Kernel statistics: rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_postprocessing.py --no-host --reps 3"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy on MI355X (MI355X_MICROARCH: HBM3E peak BW row)
# per voxel and class entry: local (seg 1 B read, labels + sizes 8 B written), merge (brick faces: a quarter of the voxels,
# two 4 B reads), flatten (labels read + written), count (sizes read), removal (labels read, seg read + written)
BYTES_PER_VOXEL_PER_ENTRY = {'local': 9, 'merge': 2, 'flatten': 8, 'count': 4, 'remove': 6}


def make_volume(n, seed=0):
    rng = np.random.default_rng(seed)
    img = np.zeros((n, n, n), np.uint8)
    z, y, x = np.ogrid[:n, :n, :n]
    for lab, c, r in ((1, (0.35, 0.3, 0.3), (0.22, 0.2, 0.18)), (2, (0.6, 0.65, 0.35), (0.18, 0.16, 0.2)),
                      (3, (0.4, 0.5, 0.75), (0.12, 0.15, 0.12))):
        m = ((z - c[0] * n) / (r[0] * n)) ** 2 + ((y - c[1] * n) / (r[1] * n)) ** 2 + ((x - c[2] * n) / (r[2] * n)) ** 2 <= 1
        img[m] = lab
    for _ in range(300):                                        # spurious blobs
        s = int(rng.integers(2, 7))
        p = [int(rng.integers(0, n - s)) for _ in range(3)]
        img[p[0]:p[0] + s, p[1]:p[1] + s, p[2]:p[2] + s] = int(rng.integers(1, 4))
    d0 = int(0.8 * n)                                           # percolation slab
    slab = rng.random((n - d0, n, n)) < 0.3116
    img[d0:][slab] = rng.integers(1, 4, int(slab.sum())).astype(np.uint8)
    return img


def host_reference(image, classes, vpv):
    """the reference's loop with scipy: label, sizes, keep every component of the largest size, zero the rest"""
    from scipy.ndimage import label
    for c in classes:
        mask = image == c
        lmap, n = label(mask.astype(int))
        if n == 0:
            continue
        sizes = np.bincount(lmap.ravel())[1:] * vpv
        drop = np.flatnonzero(sizes != sizes.max()) + 1
        image[np.isin(lmap, drop) & mask] = 0
    return image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from multitalent_amd.postprocessing.connected_components import remove_all_but_the_largest_connected_component
    n, vpv, classes = a.size, 0.8 * 0.8 * 1.5, [1, 2, 3]
    img = make_volume(n)
    src = torch.from_numpy(img).cuda()
    work = torch.empty_like(src)
    times = []
    for it in range(a.reps + 1):                                # the first call is the warm-up
        work.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        remove_all_but_the_largest_connected_component(work, classes, vpv)
        e1.record()
        torch.cuda.synchronize()
        if it:
            times.append(e0.elapsed_time(e1))
    dev_out = work.cpu().numpy()
    V = n ** 3
    per_entry = sum(BYTES_PER_VOXEL_PER_ENTRY.values()) * V
    bound_ms = per_entry * len(classes) / HBM_BYTES_PER_S * 1e3
    res = {'metric': 'remove_all_but_the_largest_connected_component %d^3, classes %s' % (n, classes),
           'device_ms_median': float(np.median(times)), 'device_ms_min': float(np.min(times)), 'reps': a.reps,
           'algorithmic_bytes_per_entry': per_entry, 'bytes_per_voxel_per_entry': BYTES_PER_VOXEL_PER_ENTRY,
           'hbm_bound_ms': bound_ms, 'share_of_hbm_bound': bound_ms / float(np.median(times)),
           'foreground_voxels': int((img > 0).sum()), 'removed_voxels': int(((img > 0) & (dev_out == 0)).sum())}
    if not a.no_host:
        ref = img.copy()
        t0 = time.perf_counter()
        host_reference(ref, classes, vpv)
        res['host_scipy_s'] = time.perf_counter() - t0
        res['identical'] = bool(np.array_equal(ref, dev_out))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if not a.no_host and not res['identical']:
        sys.exit(1)


if __name__ == '__main__':
    main()
