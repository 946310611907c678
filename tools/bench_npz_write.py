"""The .npz writer: stored float16 probabilities (3 and 15 channels of 180 x 512 x 512) and a float32 training case (2 x 180 x 512 x
512), each written by the device writer (utilities.npz_io.save_npz_device: DEFLATE at the element size on the device, only
compressed bytes come back) and by the former path (`.cpu().numpy()` + `np.savez_compressed`, zlib level 6 on one thread), in
alternating runs on the same machine.  Per input: seconds per stage (encode = both passes, table construction and launches;
read-back + CRC join; file write), the encoder's bandwidth in input bytes/s, file bytes on both sides.  Medians and raw runs ->
--out (json; an existing file is extended, so the inputs can be measured in separate invocations)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch


def _ellipsoid(shape, centre, radii, dev):
    g = [torch.arange(s, device=dev, dtype=torch.float32) for s in shape]
    return sum((((g[a] - centre[a] * shape[a]) / (radii[a] * shape[a])) ** 2).reshape([-1 if i == a else 1 for i in range(3)]) for a in range(3))


def probabilities(C, shape, dev, seed=0):
    """float16 softmax over C classes: smooth blobs with noisy logits, saturated to exactly 0 / 1 away from the class borders"""
    rs = np.random.RandomState(seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    logits = torch.empty((C,) + shape, device=dev)
    for c in range(C):
        logits[c] = 14 * (1 - _ellipsoid(shape, rs.uniform(0.25, 0.75, 3), rs.uniform(0.15, 0.4, 3), dev)).clamp_(-3, 1)
        logits[c] += torch.randn(shape, device=dev, generator=g)
    return torch.softmax(logits, 0).half()


def training_case(shape, dev, seed=0):
    """float32 [2, X, Y, Z]: normalised data that is zero outside the body mask, and the label channel (-1 outside, 0..3 inside)"""
    rs = np.random.RandomState(seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    body = _ellipsoid(shape, (0.5, 0.5, 0.5), (0.45, 0.4, 0.4), dev) <= 1
    out = torch.zeros((2,) + shape, device=dev)
    out[0] = torch.randn(shape, device=dev, generator=g) * body
    out[1] = torch.where(body, 0.0, -1.0)
    for lab in range(1, 4):
        out[1][(_ellipsoid(shape, rs.uniform(0.4, 0.6, 3), rs.uniform(0.05, 0.15, 3), dev) <= 1) & body] = lab
    return out


INPUTS = {'float16 probabilities 3ch': lambda s, d: ('softmax', probabilities(3, s, d)),
          'float16 probabilities 15ch': lambda s, d: ('softmax', probabilities(15, s, d)),
          'float32 training case': lambda s, d: ('data', training_case(s, d))}


def _device_write(key, t, fname):
    from multitalent_amd.utilities.npz_io import save_npz_device
    st = {}
    t0 = time.perf_counter()
    save_npz_device(fname, _stages=st, **{key: t})
    total = time.perf_counter() - t0
    return {'encode': st['encode'], 'readback': st['readback'], 'file': total - st['encode'] - st['readback'], 'total': total}


def _former_write(key, t, fname):
    t0 = time.perf_counter()
    arr = t.cpu().numpy()
    t1 = time.perf_counter()
    np.savez_compressed(fname, **{key: arr})
    return {'copy': t1 - t0, 'zlib+file': time.perf_counter() - t1, 'total': time.perf_counter() - t0}


def main(names, shape, reps, out_file):
    dev = torch.device('cuda:0')
    result = {'shape': list(shape), 'reps': reps, 'inputs': {}, 'lines': []}
    if out_file and os.path.isfile(out_file):
        with open(out_file) as f:
            result = json.load(f)
    tmp = tempfile.mkdtemp()
    f_dev, f_old = os.path.join(tmp, 'dev.npz'), os.path.join(tmp, 'old.npz')
    for name in names:
        key, t = INPUTS[name](shape, dev)
        torch.cuda.synchronize()
        _device_write(key, t[:1], f_dev)                                  # warm-up: library load, allocator
        runs = {'device': [], 'former': []}
        for r in range(reps):                                             # alternating runs
            torch.cuda.synchronize(); runs['device'].append(_device_write(key, t, f_dev))
            torch.cuda.synchronize(); runs['former'].append(_former_write(key, t, f_old))
            print('  %s run %d: device %.3f s, former %.1f s' % (name, r, runs['device'][-1]['total'], runs['former'][-1]['total']), flush=True)
        a, b = np.load(f_dev)[key], np.load(f_old)[key]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        med = {k: {s: float(np.median([x[s] for x in v])) for s in v[0]} for k, v in runs.items()}
        sizes = {'device': os.path.getsize(f_dev), 'numpy': os.path.getsize(f_old)}
        nbytes = t.numel() * t.element_size() + 128
        entry = {'median_s': med, 'runs': runs, 'file_bytes': sizes, 'input_bytes': nbytes, 'saturated': float(((t == 0) | (t == 1)).float().mean()),
                 'encoder_GBps': nbytes / med['device']['encode'] / 1e9, 'size_ratio': sizes['device'] / sizes['numpy']}
        result['inputs'][name] = entry
        line = ('%s %s: device %.1f ms (encode %.1f, read-back + CRC join %.1f, file %.1f; %.1f GB/s of input) vs former %.2f s (copy %.2f, '
                'zlib 6 + file %.2f); %d vs %d bytes (%.2f)' % (name, tuple(t.shape), med['device']['total'] * 1e3, med['device']['encode'] * 1e3,
                                                               med['device']['readback'] * 1e3, med['device']['file'] * 1e3, entry['encoder_GBps'],
                                                               med['former']['total'], med['former']['copy'], med['former']['zlib+file'],
                                                               sizes['device'], sizes['numpy'], entry['size_ratio']))
        result['lines'] = [x for x in result['lines'] if not x.startswith(name + ' ')] + [line]
        print(line, flush=True)
        del t
        torch.cuda.empty_cache()
        if out_file:
            os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
            with open(out_file, 'w') as f:
                json.dump(result, f, indent=1)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--inputs', nargs='*', default=list(INPUTS), choices=list(INPUTS))
    ap.add_argument('--shape', type=int, nargs=3, default=(180, 512, 512))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='json file (profiles/npz_write_bench.json)')
    a = ap.parse_args()
    main(a.inputs, tuple(a.shape), a.reps, a.out)
