"""Timing of the dataset conversion's label step (`copy_and_convert_segmentation_nifti`) on the device against a numpy restatement
of the reference's function.

Seeded blocky label volumes of 180 x 512 x 512 and 512^3 voxels with 2 and 13 labels, stored as uint8, int16 and float64 `.nii.gz`
files.  Per (shape, labels, dtype):
  * the kernel `mt_label_convert` alone: device events around --reps back-to-back launches on the uploaded volume, its minimum
    traffic (itemsize + 1) * V bytes, the bandwidth that gives and its share of the 6.29 TB/s float4 streaming figure of DESIGN;
  * the whole per-file call split into read + decompress, upload, kernel (with the read-back of its report), download, and
    compress + write (wall clock around work that ends in a synchronise);
  * the host leg: the reference's algorithm restated with numpy (np.unique, the `> 1e-20` filter, the membership check, one masked
    assignment per label) on the float64 array `get_fdata` would return, cast included; its result must equal the device's or the
    tool exits 1.
Reading, decompressing, compressing and writing are host work on both sides and are reported separately, not hidden in a ratio.
One JSON line per configuration, all of them written to --out.

Run: python tools/bench_dataset_conversion.py [--shapes ct180,cube512] [--labels 2,13] [--dtypes uint8,int16,float64] [--reps 20]
     [--workdir DIR] [--out profiles/dataset_conversion_bench.json]"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

SHAPES = {'ct180': (180, 512, 512), 'cube512': (512, 512, 512)}
STREAM_TBS = 6.29


def make_volume(shape, nlabels, dtype, seed):
    rng = np.random.default_rng(seed)
    seg = np.zeros(shape, dtype=dtype)
    for lab in range(1, nlabels + 1):
        sz = [max(4, int(n / 3 * rng.uniform(0.4, 1.0))) for n in shape]
        lo = [int(rng.integers(0, n - s + 1)) for n, s in zip(shape, sz)]
        seg[lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = lab
    return seg


def host_reference(a, labels_in, labels_out):
    """The reference's steps, restated: -> (uint8 volume, seconds for the float64 cast, seconds for the rest)."""
    t0 = time.perf_counter()
    seg = np.ascontiguousarray(a.astype(np.float64))
    t1 = time.perf_counter()
    uniques = np.unique(seg)
    uniques = uniques[uniques > 1e-20]
    known = np.unique(labels_in)
    for u in uniques:
        if u not in known:
            raise RuntimeError("unexpected label %r" % u)
    out = np.zeros(seg.shape, dtype=np.uint8)
    for i, o in zip(labels_in, labels_out):
        if i in uniques:
            out[seg == i] = o
    return out, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='ct180,cube512')
    ap.add_argument('--labels', default='2,13')
    ap.add_argument('--dtypes', default='uint8,int16,float64')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--no_host', action='store_true', help="skip the host leg")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dataset_conversion_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset_conversion: no HIP device; nothing is measured without one")
    from multitalent_amd import _lib, ops
    from multitalent_amd.dataset_conversion.Task100_MultiTalent import label_table
    from multitalent_amd.utilities.nifti_io import read_image, write_image
    lib = _lib.load()
    work = a.workdir or tempfile.mkdtemp(prefix='bench_conversion_')
    os.makedirs(work, exist_ok=True)
    lines = []
    try:
        for sname in a.shapes.split(','):
            shape = SHAPES[sname]
            V = int(np.prod(shape))
            for nl in (int(i) for i in a.labels.split(',')):
                labels_in, labels_out = tuple(range(1, nl + 1)), tuple(range(10, 10 + nl))
                table = label_table(labels_in, labels_out)
                for dt in a.dtypes.split(','):
                    src, dst = os.path.join(work, 'in.nii.gz'), os.path.join(work, 'out.nii.gz')
                    write_image(make_volume(shape, nl, dt, 7 * nl + len(dt)), src, (0.8, 0.8, 2.5))
                    t0 = time.perf_counter()
                    img = read_image(src)
                    arr = np.ascontiguousarray(np.asarray(img.array))
                    t_read = time.perf_counter() - t0
                    assert arr.dtype.name == dt
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    seg = torch.from_numpy(arr).cuda()
                    torch.cuda.synchronize()
                    t_up = time.perf_counter() - t0
                    ops.label_convert(seg, table)                                  # warm-up: code object, allocator
                    t0 = time.perf_counter()
                    out, count, _ = ops.label_convert(seg, table)
                    torch.cuda.synchronize()
                    t_kernel_call = time.perf_counter() - t0
                    assert count == 0
                    t0 = time.perf_counter()
                    host_out = out.cpu().numpy()
                    t_down = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    write_image(host_out, dst, img.GetSpacing(), img.GetOrigin(), img.GetDirection())
                    t_write = time.perf_counter() - t0
                    # the kernel alone
                    report = torch.empty(2, dtype=torch.int64, device=seg.device)
                    tp = table.ctypes.data_as(C.POINTER(C.c_uint16))
                    code = ops.LABEL_CONVERT_DTYPES[dt]
                    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                    launch = lambda: _lib.check(lib.mt_label_convert(C.c_void_p(seg.data_ptr()), code, V, tp, C.c_void_p(out.data_ptr()),
                                                                     C.c_void_p(report.data_ptr()), stream), 'label_convert')
                    for _ in range(3):
                        launch()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        launch()
                    e1.record()
                    torch.cuda.synchronize()
                    k_ms = e0.elapsed_time(e1) / a.reps
                    traffic = (arr.dtype.itemsize + 1) * V
                    rec = {'shape': sname, 'voxels': V, 'labels': nl, 'dtype': dt, 'file_bytes': os.path.getsize(src),
                           'kernel_ms': k_ms, 'kernel_min_traffic_bytes': traffic, 'kernel_TBs': traffic / (k_ms * 1e-3) / 1e12,
                           'kernel_share_of_%.2f_TBs' % STREAM_TBS: traffic / (k_ms * 1e-3) / 1e12 / STREAM_TBS,
                           'kernel_bound_ms_at_%.2f_TBs' % STREAM_TBS: traffic / (STREAM_TBS * 1e12) * 1e3,
                           'volume_fits_256MB_last_level_cache': traffic < 256 * 2 ** 20,
                           'call_s': {'read_decompress': t_read, 'upload': t_up, 'kernel_and_report': t_kernel_call, 'download': t_down,
                                      'compress_write': t_write, 'total': t_read + t_up + t_kernel_call + t_down + t_write}}
                    if not a.no_host:
                        want, t_cast, t_rest = host_reference(arr, labels_in, labels_out)
                        rec['host_s'] = {'float64_cast': t_cast, 'unique_check_assign': t_rest, 'total': t_cast + t_rest}
                        if not np.array_equal(want, host_out):
                            print("MISMATCH between the device and the host leg for", sname, nl, dt)
                            raise SystemExit(1)
                        del want
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                    del seg, out, arr, img, host_out
                    torch.cuda.empty_cache()
    finally:
        if a.workdir is None:
            shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
