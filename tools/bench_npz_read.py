"""The readers: the three inputs of tools/bench_npz_write.py (stored float16 probabilities of 3 and 15 channels, a float32 training
case, 180 x 512 x 512) and a 512^3 uint8 label map as .nii.gz, each written by the device writer; an incompressible uint8 volume
(every chunk stored) written by the device writer; and the training case written by `np.savez_compressed` (no restart points: the
reader's fallback).  Each is read by the device reader (utilities.npz_io.load_npz_device / utilities.nifti_io.read_image_device:
compressed bytes uploaded, inflated on the device) and by the former path (`np.load(...)[key]` / `_read_nifti`, zlib on one host
thread, then an upload), in alternating runs on the same machine.  Per input: seconds per stage (file read, upload, scan, write,
CRC + header), GB/s of output on both sides.  Medians and raw runs -> --out (json; an existing file is extended)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, HERE)
import numpy as np
import torch

from bench_npz_write import probabilities, training_case


def label_map(shape, dev, seed=0):
    from bench_npz_write import _ellipsoid
    rs = np.random.RandomState(seed)
    out = torch.zeros(shape, dtype=torch.uint8, device=dev)
    for lab in range(1, 6):
        out[_ellipsoid(shape, rs.uniform(0.3, 0.7, 3), rs.uniform(0.05, 0.25, 3), dev) <= 1] = lab
    return out


def noise(shape, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)


# name -> (kind, key, generator, writer: 'device' or 'numpy', shape or None for --shape)
INPUTS = {'float16 probabilities 3ch': ('npz', 'softmax', lambda s, d: probabilities(3, s, d), 'device', None),
          'float16 probabilities 15ch': ('npz', 'softmax', lambda s, d: probabilities(15, s, d), 'device', None),
          'float32 training case': ('npz', 'data', lambda s, d: training_case(s, d), 'device', None),
          'uint8 label map 512^3 .nii.gz': ('nii', None, label_map, 'device', (512, 512, 512)),
          'uint8 noise (all chunks stored)': ('npz', 'data', noise, 'device', (256, 512, 512)),
          'float32 training case, np.savez_compressed': ('npz', 'data', lambda s, d: training_case(s, d), 'numpy', None)}


def _device_read(kind, key, fname, dev):
    from multitalent_amd.utilities.nifti_io import read_image_device
    from multitalent_amd.utilities.npz_io import load_npz_device
    st = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t = load_npz_device(fname, key, dev, stages=st) if kind == 'npz' else read_image_device(fname, dev, st)[0]
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    out = {k: float(st.get(k, 0.0)) for k in ('file', 'upload', 'scan', 'write')}
    out['crc+header'] = float(st.get('crc', 0.0) + st.get('header', 0.0))
    out['total'] = total
    return t, st['path'], out


def _former_read(kind, key, fname, dev):
    from multitalent_amd.utilities.nifti_io import _read_nifti
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arr = np.load(fname)[key] if kind == 'npz' else _read_nifti(fname).array
    t1 = time.perf_counter()
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    torch.cuda.synchronize()
    return t, {'file+zlib': t1 - t0, 'upload': time.perf_counter() - t1, 'total': time.perf_counter() - t0}


def main(names, shape, reps, out_file):
    from multitalent_amd.utilities.nifti_io import write_label_map_device
    from multitalent_amd.utilities.npz_io import save_npz_device
    dev = torch.device('cuda:0')
    result = {'shape': list(shape), 'reps': reps, 'inputs': {}, 'lines': []}
    if out_file and os.path.isfile(out_file):
        with open(out_file) as f:
            result = json.load(f)
    tmp = tempfile.mkdtemp()
    for name in names:
        kind, key, make, writer, own_shape = INPUTS[name]
        t = make(tuple(own_shape or shape), dev)
        fname = os.path.join(tmp, 'in.npz' if kind == 'npz' else 'in.nii.gz')
        if kind == 'nii':
            write_label_map_device(t, fname, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
        elif writer == 'device':
            save_npz_device(fname, **{key: t})
        else:
            np.savez_compressed(fname, **{key: t.cpu().numpy()})
        nbytes = t.numel() * t.element_size()
        want = t.reshape(-1).view(torch.uint8)
        runs, path = {'device': [], 'former': []}, None
        _device_read(kind, key, fname, dev)                               # warm-up: library load, allocator, page cache
        for r in range(reps):                                             # alternating runs
            a, path, d = _device_read(kind, key, fname, dev)
            assert torch.equal(a.reshape(-1).view(torch.uint8), want)
            del a
            b, f = _former_read(kind, key, fname, dev)
            assert torch.equal(b.reshape(-1).view(torch.uint8), want)
            del b
            runs['device'].append(d); runs['former'].append(f)
            print('  %s run %d: device reader (%s path) %.3f s, former %.3f s' % (name, r, path, d['total'], f['total']), flush=True)
        med = {k: {s: float(np.median([x[s] for x in v])) for s in v[0]} for k, v in runs.items()}
        entry = {'median_s': med, 'runs': runs, 'path': path, 'file_bytes': os.path.getsize(fname), 'output_bytes': nbytes,
                 'device_GBps': nbytes / med['device']['total'] / 1e9, 'former_GBps': nbytes / med['former']['total'] / 1e9,
                 'speedup': med['former']['total'] / med['device']['total']}
        result['inputs'][name] = entry
        m = med['device']
        line = ('%s %s (%d -> %d bytes): device reader (%s path) %.1f ms (file %.1f, upload %.1f, scan %.1f, write %.1f, CRC + header %.1f; '
                '%.2f GB/s of output) vs np.load / gzip + upload %.1f ms (file + zlib %.1f, upload %.1f; %.2f GB/s): %.1fx'
                % (name, tuple(t.shape), entry['file_bytes'], nbytes, path, m['total'] * 1e3, m['file'] * 1e3, m['upload'] * 1e3, m['scan'] * 1e3,
                   m['write'] * 1e3, m['crc+header'] * 1e3, entry['device_GBps'], med['former']['total'] * 1e3, med['former']['file+zlib'] * 1e3,
                   med['former']['upload'] * 1e3, entry['former_GBps'], entry['speedup']))
        result['lines'] = [x for x in result['lines'] if not x.startswith(name + ' (')] + [line]
        print(line, flush=True)
        del t, want
        torch.cuda.empty_cache()
        if out_file:
            os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
            with open(out_file, 'w') as f:
                json.dump(result, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs', nargs='*', default=list(INPUTS), choices=list(INPUTS))
    ap.add_argument('--shape', type=int, nargs=3, default=(180, 512, 512))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='json file (profiles/npz_read_bench.json)')
    a = ap.parse_args()
    main(a.inputs, tuple(a.shape), a.reps, a.out)
