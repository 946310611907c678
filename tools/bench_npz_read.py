"""The readers: the three inputs of tools/bench_npz_write.py (stored float16 probabilities of 3 and 15 channels, a float32 training
case, 180 x 512 x 512) and a 512^3 uint8 label map as .nii.gz, each written by the device writer; an incompressible uint8 volume
(every chunk stored) written by the device writer; and the training case written by `np.savez_compressed` (no restart points: the
reader's fallback).  Each is read by the device reader (utilities.npz_io.load_npz_device / utilities.nifti_io.read_image_device:
compressed bytes uploaded, inflated on the device) and by the former path (`np.load(...)[key]` / `_read_nifti`, zlib on one host
thread, then an upload), in alternating runs on the same machine.  Per input: seconds per stage (file read, upload, scan, write,
CRC + header), GB/s of output on both sides.  Medians and raw runs -> --out (json; an existing file is extended).

Files of other writers, which the readers decode from block starts they search in the stream (ops.inflate_stream): the
training case and 15-channel float16 probabilities written by `np.savez_compressed`, an int16 180 x 512 x 512 CT and a 512^3 uint8
label map as .nii.gz at gzip level 6, and the same CT cut by Z_SYNC_FLUSH every 128 KiB as pigz cuts it.  For these the stage
times are search, size, chain, symbols, windows and resolve, and the unit count is reported.
--sweep-chunk times ops.inflate_stream alone on each of those streams for chunks of 2 .. 64 KiB (what INFLATE_SPEC_CHUNK is chosen
from); --threshold reads gzip-6 CT files of 2 MiB, 4 MiB, ... through both paths, alternating, and reports the smallest size at
which the device route's median is at most 0.8 of the former path's (what INFLATE_SPEC_MIN_OUT is chosen from)."""
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


def ct_volume(shape, dev, seed=0):
    """CT-like int16: smooth structures plus a little noise, as a scanner's"""
    from bench_npz_write import _ellipsoid
    rs = np.random.RandomState(seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.full(shape, -1000.0, device=dev)
    for _ in range(12):
        e = _ellipsoid(shape, rs.uniform(0.3, 0.7, 3), rs.uniform(0.1, 0.35, 3), dev)
        out = torch.where(e <= 1, out + float(rs.uniform(100, 500)) * (1 - e), out)
    out += torch.randn(shape, device=dev, generator=g) * 8
    return out.round().clamp(-1024, 3000).to(torch.int16)


def noise(shape, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)


# name -> (kind, key, generator, writer: 'device' or 'numpy', shape or None for --shape)
INPUTS = {'float16 probabilities 3ch': ('npz', 'softmax', lambda s, d: probabilities(3, s, d), 'device', None),
          'float16 probabilities 15ch': ('npz', 'softmax', lambda s, d: probabilities(15, s, d), 'device', None),
          'float32 training case': ('npz', 'data', lambda s, d: training_case(s, d), 'device', None),
          'uint8 label map 512^3 .nii.gz': ('nii', None, label_map, 'device', (512, 512, 512)),
          'uint8 noise (all chunks stored)': ('npz', 'data', noise, 'device', (256, 512, 512)),
          'float32 training case, np.savez_compressed': ('npz', 'data', lambda s, d: training_case(s, d), 'numpy', None),
          'float16 probabilities 15ch, np.savez_compressed': ('npz', 'softmax', lambda s, d: probabilities(15, s, d), 'numpy', None),
          'int16 CT .nii.gz, gzip 6': ('nii', None, ct_volume, 'gzip6', (180, 512, 512)),
          'uint8 label map 512^3 .nii.gz, gzip 6': ('nii', None, label_map, 'gzip6', (512, 512, 512)),
          'int16 CT .nii.gz, sync flush every 128 KiB': ('nii', None, ct_volume, 'sync128k', (180, 512, 512))}
FOREIGN = [k for k, v in INPUTS.items() if v[3] != 'device']
SPEC_STAGES = ('search', 'size', 'chain', 'symbols', 'windows', 'resolve')


def write_foreign_nifti(t, fname, writer):
    """the volume as another writer's .nii.gz: gzip level 6, whole or cut by Z_SYNC_FLUSH every 128 KiB"""
    import gzip
    import zlib
    from multitalent_amd.utilities import deflate_host
    from multitalent_amd.utilities.nifti_io import _nifti_header
    arr = t.cpu().numpy()
    plain = _nifti_header(arr.shape, arr.dtype, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel())) + arr.tobytes()
    if writer == 'gzip6':
        blob = gzip.compress(plain, 6)
    else:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = b''.join(c.compress(plain[i:i + (128 << 10)]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(plain), 128 << 10)) + c.flush()
        blob = deflate_host.gzip_member(body, zlib.crc32(plain), len(plain))
    with open(fname, 'wb') as f:
        f.write(blob)


def _device_read(kind, key, fname, dev):
    from multitalent_amd.utilities.nifti_io import read_image_device
    from multitalent_amd.utilities.npz_io import load_npz_device
    st = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t = load_npz_device(fname, key, dev, stages=st) if kind == 'npz' else read_image_device(fname, dev, st)[0]
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    out = {k: float(st.get(k, 0.0)) for k in ('file', 'upload', 'scan', 'write') + SPEC_STAGES}
    out['crc+header'] = float(st.get('crc', 0.0) + st.get('header', 0.0))
    out['total'] = total
    return t, (st['path'], st.get('route'), st.get('units')), out


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
        if kind == 'nii' and writer != 'device':
            write_foreign_nifti(t, fname, writer)
        elif kind == 'nii':
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
            a, (path, route, units), d = _device_read(kind, key, fname, dev)
            assert torch.equal(a.reshape(-1).view(torch.uint8), want)
            del a
            b, f = _former_read(kind, key, fname, dev)
            assert torch.equal(b.reshape(-1).view(torch.uint8), want)
            del b
            runs['device'].append(d); runs['former'].append(f)
            print('  %s run %d: device reader (%s path) %.3f s, former %.3f s' % (name, r, path, d['total'], f['total']), flush=True)
        med = {k: {s: float(np.median([x[s] for x in v])) for s in v[0]} for k, v in runs.items()}
        entry = {'median_s': med, 'runs': runs, 'path': path, 'route': route, 'units': units, 'file_bytes': os.path.getsize(fname), 'output_bytes': nbytes,
                 'device_GBps': nbytes / med['device']['total'] / 1e9, 'former_GBps': nbytes / med['former']['total'] / 1e9,
                 'speedup': med['former']['total'] / med['device']['total']}
        result['inputs'][name] = entry
        m = med['device']
        line = ('%s %s (%d -> %d bytes): device reader (%s path) %.1f ms (file %.1f, upload %.1f, scan %.1f, write %.1f, CRC + header %.1f; '
                '%.2f GB/s of output) vs np.load / gzip + upload %.1f ms (file + zlib %.1f, upload %.1f; %.2f GB/s): %.1fx'
                % (name, tuple(t.shape), entry['file_bytes'], nbytes, path, m['total'] * 1e3, m['file'] * 1e3, m['upload'] * 1e3, m['scan'] * 1e3,
                   m['write'] * 1e3, m['crc+header'] * 1e3, entry['device_GBps'], med['former']['total'] * 1e3, med['former']['file+zlib'] * 1e3,
                   med['former']['upload'] * 1e3, entry['former_GBps'], entry['speedup']))
        if route == 'speculative':
            line += ('; speculative route, %d units: search %.1f, size %.1f, chain %.1f, symbols %.1f, windows %.1f, resolve %.1f ms'
                     % ((units,) + tuple(m[k] * 1e3 for k in SPEC_STAGES)))
        result['lines'] = [x for x in result['lines'] if not x.startswith(name + ' (')] + [line]
        print(line, flush=True)
        del t, want
        torch.cuda.empty_cache()
        if out_file:
            os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
            with open(out_file, 'w') as f:
                json.dump(result, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)


def _save(result, out_file):
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        with open(out_file, 'w') as f:
            json.dump(result, f, indent=1)


def _load(out_file):
    if out_file and os.path.isfile(out_file):
        with open(out_file) as f:
            return json.load(f)
    return {'inputs': {}, 'lines': []}


def _raw_stream(kind, key, fname):
    """the member's raw DEFLATE stream and its size, as the readers cut it out of the file"""
    from multitalent_amd.utilities.nifti_io import gzip_payload
    from multitalent_amd.utilities.npz_io import locate_member
    blob = open(fname, 'rb').read()
    if kind == 'npz':
        m = locate_member(fname, key)
        return blob[m['offset']:m['offset'] + m['csize']], m['usize']
    p, n, _, isize = gzip_payload(blob, fname)
    return blob[p:p + n], None


def sweep_chunk(names, shape, reps, out_file):
    """ops.inflate_stream alone (stream on the device, output not read back) per chunk size"""
    from multitalent_amd import ops
    dev = torch.device('cuda:0')
    result = _load(out_file)
    sweep = result.setdefault('spec_chunk_sweep', {})
    tmp = tempfile.mkdtemp()
    for name in names:
        kind, key, make, writer, own_shape = INPUTS[name]
        t = make(tuple(own_shape or shape), dev)
        fname = os.path.join(tmp, 'in.npz' if kind == 'npz' else 'in.nii.gz')
        if kind == 'nii':
            write_foreign_nifti(t, fname, writer)
        else:
            np.savez_compressed(fname, **{key: t.cpu().numpy()})
        del t
        body, n_out = _raw_stream(kind, key, fname)
        comp = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).to(dev)
        row = {}
        for lg in range(11, 17):
            times, info = [], None
            for r in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    out, _, info = ops.inflate_stream(comp, n_out=n_out, chunk=1 << lg)
                except ops.InflateForeign as e:
                    info = e.info
                    break
                torch.cuda.synchronize()
                if r:
                    times.append(time.perf_counter() - t0)
                del out
            row[str(1 << lg)] = {'median_s': float(np.median(times)) if times else None, 'status': info['status'], 'units': info['units'],
                                 'candidates': info['candidates']}
            print('  %s chunk %d: %s' % (name, 1 << lg, row[str(1 << lg)]), flush=True)
        sweep[name] = row
        del comp
        torch.cuda.empty_cache()
        _save(result, out_file)
    shutil.rmtree(tmp, ignore_errors=True)


def threshold(reps, out_file, sizes):
    """gzip-6 CT files of 2^k output bytes through the device reader with the threshold taken away, and through the former path"""
    from multitalent_amd import ops
    dev = torch.device('cuda:0')
    result = _load(out_file)
    rows = result.setdefault('spec_threshold', {})
    tmp = tempfile.mkdtemp()
    keep, ops.INFLATE_SPEC_MIN_OUT = ops.INFLATE_SPEC_MIN_OUT, 0
    try:
        for size in sizes:
            z = max(1, (size - 352) // (2 * 256 * 256))
            t = ct_volume((z, 256, 256), dev, seed=z)
            fname = os.path.join(tmp, 'in.nii.gz')
            write_foreign_nifti(t, fname, 'gzip6')
            _device_read('nii', None, fname, dev)
            d, f, tag = [], [], None
            for r in range(reps):
                a, tag, dd = _device_read('nii', None, fname, dev)
                b, ff = _former_read('nii', None, fname, dev)
                assert torch.equal(a, b)
                d.append(dd['total']); f.append(ff['total'])
            rows[str(size)] = {'device_s': d, 'former_s': f, 'device_median_s': float(np.median(d)), 'former_median_s': float(np.median(f)),
                               'ratio': float(np.median(d) / np.median(f)), 'path': tag[0], 'route': tag[1], 'units': tag[2]}
            print('  threshold %d bytes: %s' % (size, {k: v for k, v in rows[str(size)].items() if not k.endswith('_s') or 'median' in k}), flush=True)
            _save(result, out_file)
    finally:
        ops.INFLATE_SPEC_MIN_OUT = keep
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs', nargs='*', default=list(INPUTS), choices=list(INPUTS))
    ap.add_argument('--shape', type=int, nargs=3, default=(180, 512, 512))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='json file (profiles/npz_read_bench.json)')
    ap.add_argument('--sweep-chunk', action='store_true', help='time ops.inflate_stream per chunk size on the inputs of other writers')
    ap.add_argument('--threshold', type=int, nargs='*', default=None, metavar='LOG2', help='output sizes 2^LOG2 to read through both paths')
    a = ap.parse_args()
    if a.sweep_chunk:
        sweep_chunk([n for n in a.inputs if n in FOREIGN], tuple(a.shape), a.reps, a.out)
    elif a.threshold is not None:
        threshold(a.reps, a.out, [1 << k for k in (a.threshold or range(21, 28))])
    else:
        main(a.inputs, tuple(a.shape), a.reps, a.out)
