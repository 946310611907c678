"""Export post-processing: device time for a 47-channel probability volume resampled to the original grid and classified, next to
the CPU restatement of the reference path timed on a bounded sample (a few channels, extrapolated linearly to 47).

--write: the file writer instead.  One 512^3 binary mask, one 512^3 multi-label map and the 47-region export of one 512^3 case
through predict_cases' loop, each written as .nii.gz by the device encoder (ops.deflate_gzip behind
utilities.nifti_io.write_label_map_device) and by the former path (voxels to the host, `_write_nifti` = Python gzip level 1), in
alternating runs on the same machine.  Per input: seconds per stage (encode launches + table construction, read-back, file write),
encoder bandwidth in input bytes/s, file sizes against the gzip level 1 file.  Medians and raw lines -> --out (json)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch


def resample_leg():
    from multitalent_amd.inference.segmentation_export import resample_and_classify
    from oracle.reference_ops import resample_probabilities
    C, src, dst = 47, (320, 320, 320), (512, 512, 512)
    dev = torch.device('cuda:0')
    p = torch.rand((C,) + src, device=dev)
    props = {'size_after_cropping': np.array(dst), 'original_size_of_raw_data': np.array(dst), 'crop_bbox': [[0, dst[i]] for i in range(3)],
             'original_spacing': np.array([1.0, 0.78, 0.78]), 'spacing_after_resampling': np.array([1.5, 1.5, 1.5])}
    order = list(range(1, C + 1))
    for sep, name in ((None, 'trilinear'), (True, 'separate z')):
        pr = dict(props)
        if sep:
            pr['original_spacing'] = np.array([5.0, 0.78, 0.78])
        resample_and_classify(p, pr, order); torch.cuda.synchronize()
        t = time.time()
        for _ in range(3):
            resample_and_classify(p, pr, order)
        torch.cuda.synchronize()
        print('%s: %d x %s -> %s uint8 on the device: %.1f ms' % (name, C, src, dst, (time.time() - t) / 3 * 1e3))
    nc = 2
    x = p[:nc].cpu().numpy()
    t = time.time()
    resample_probabilities(x, dst, axis=None, do_separate_z=False)
    dt = time.time() - t
    print('CPU restatement (scipy zoom order 1, 1 core): %.1f s for %d channels -> %.0f s for %d channels (+ thresholds)' % (dt, nc, dt / nc * C, C))


GEO = ((0.78, 0.78, 1.0), (0.0, 0.0, 0.0), (1, 0, 0, 0, 1, 0, 0, 0, 1))


def _ellipsoid(shape, centre, radii, dev):
    g = [torch.arange(s, device=dev, dtype=torch.float32) for s in shape]
    return sum((((g[a] - centre[a] * shape[a]) / (radii[a] * shape[a])) ** 2).reshape([-1 if i == a else 1 for i in range(3)]) for a in range(3))


def _former_write(seg_dev, fname):
    """what write_image did for a label map before the device encoder, without SimpleITK: copy the voxels, gzip level 1 on one thread"""
    from multitalent_amd.utilities.nifti_io import Image, _write_nifti
    t0 = time.perf_counter()
    arr = seg_dev.cpu().numpy().astype(np.uint8)
    t1 = time.perf_counter()
    _write_nifti(Image(arr, *GEO), fname)
    return {'copy': t1 - t0, 'gzip+file': time.perf_counter() - t1}


def _device_write(seg_dev, fname):
    from multitalent_amd.utilities.nifti_io import write_label_map_device
    st = {}
    write_label_map_device(seg_dev, fname, *GEO, stages=st)
    return st


def write_leg(n, reps, out_file):
    dev = torch.device('cuda:0')
    shape = (n, n, n)
    rs = np.random.RandomState(0)
    inputs = {'binary ball': (_ellipsoid(shape, (0.5, 0.5, 0.5), (0.4, 0.4, 0.4), dev) <= 1).to(torch.uint8)}
    multi = torch.zeros(shape, dtype=torch.uint8, device=dev)
    for lab in range(1, 5):
        multi[_ellipsoid(shape, rs.uniform(0.3, 0.7, 3), rs.uniform(0.1, 0.3, 3), dev) <= 1] = lab
    inputs['4-label map'] = multi
    result, lines = {'shape': list(shape), 'reps': reps, 'inputs': {}}, []
    tmp = tempfile.mkdtemp()
    f_dev, f_old = os.path.join(tmp, 'dev.nii.gz'), os.path.join(tmp, 'old.nii.gz')
    for name, seg in inputs.items():
        _device_write(seg, f_dev)                                        # warm-up: library load, allocator
        runs = {'device': [], 'former': []}
        for _ in range(reps):                                            # alternating runs
            torch.cuda.synchronize(); t = time.perf_counter(); st = _device_write(seg, f_dev); runs['device'].append(dict(st, total=time.perf_counter() - t))
            torch.cuda.synchronize(); t = time.perf_counter(); st = _former_write(seg, f_old); runs['former'].append(dict(st, total=time.perf_counter() - t))
        import gzip
        assert gzip.open(f_dev).read() == gzip.open(f_old).read()
        med = {k: {s: float(np.median([r[s] for r in v])) for s in v[0]} for k, v in runs.items()}
        sizes = {'device': os.path.getsize(f_dev), 'gzip level 1': os.path.getsize(f_old)}
        nbytes = seg.numel() + 352
        entry = {'median_s': med, 'runs': runs, 'file_bytes': sizes, 'input_bytes': nbytes,
                 'encoder_GBps': nbytes / med['device']['encode'] / 1e9, 'size_ratio': sizes['device'] / sizes['gzip level 1']}
        result['inputs'][name] = entry
        lines.append('%s %s: device %.1f ms (encode %.1f, read-back %.2f, file %.2f; %.1f GB/s of input) vs former %.1f ms (copy %.1f, gzip + file '
                     '%.1f); %d vs %d bytes (%.2f)' % (name, shape, med['device']['total'] * 1e3, med['device']['encode'] * 1e3,
                                                       med['device']['readback'] * 1e3, med['device']['file'] * 1e3, entry['encoder_GBps'],
                                                       med['former']['total'] * 1e3, med['former']['copy'] * 1e3, med['former']['gzip+file'] * 1e3,
                                                       sizes['device'], sizes['gzip level 1'], entry['size_ratio']))
        print(lines[-1], flush=True)
    # the 47 regions of one case, through the loop of predict_MultiTalent.predict_cases: resample + classify + write per region
    from multitalent_amd.inference.segmentation_export import export_label_map_device, resample_and_classify
    C, src = 47, tuple(max(8, n * 5 // 8) for _ in range(3))
    probs = torch.empty((C,) + src, device=dev)
    for c in range(C):
        probs[c] = torch.sigmoid(4 * (1 - _ellipsoid(src, rs.uniform(0.3, 0.7, 3), rs.uniform(0.05, 0.3, 3), dev)))
    props = {'size_after_cropping': np.array(shape), 'original_size_of_raw_data': np.array(shape), 'crop_bbox': [[0, n]] * 3,
             'original_spacing': np.array([1.0, 0.78, 0.78]), 'spacing_after_resampling': np.array([1.5, 1.5, 1.5]),
             'itk_spacing': GEO[0], 'itk_origin': GEO[1], 'itk_direction': GEO[2]}

    def loop_device():
        for c in range(C):
            export_label_map_device(probs[c:c + 1], os.path.join(tmp, 'd%02d.nii.gz' % c), props, 1, ((1,),))

    def loop_former():
        for c in range(C):
            _former_write(resample_and_classify(probs[c:c + 1], props, ((1,),)), os.path.join(tmp, 'o%02d.nii.gz' % c))

    runs = {'device': [], 'former': []}
    for _ in range(max(1, reps // 2)):
        for key, fn in (('device', loop_device), ('former', loop_former)):
            torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); runs[key].append(time.perf_counter() - t)
    sizes = {k: sum(os.path.getsize(os.path.join(tmp, '%s%02d.nii.gz' % (p, c))) for c in range(C)) for k, p in (('device', 'd'), ('gzip level 1', 'o'))}
    med = {k: float(np.median(v)) for k, v in runs.items()}
    result['inputs']['47 regions'] = {'median_s': med, 'runs': runs, 'file_bytes': sizes, 'probabilities': list(src)}
    lines.append('47 regions %s -> %s, resample + classify + write per region: device %.2f s vs former %.2f s per case; %d vs %d bytes (%.2f)'
                 % (src, shape, med['device'], med['former'], sizes['device'], sizes['gzip level 1'], sizes['device'] / sizes['gzip level 1']))
    print(lines[-1], flush=True)
    result['lines'] = lines
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, 'w') as f:
            json.dump(result, f, indent=1)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--write', action='store_true', help='time the .nii.gz writer instead of the resampling kernel')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='json file for the --write leg (profiles/export_write_bench.json)')
    a = ap.parse_args()
    if a.write:
        write_leg(a.size, a.reps, a.out)
    else:
        resample_leg()
