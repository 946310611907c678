"""Timing of the ensemble merge on the device (`inference.ensemble_predictions.merge_files` over `mt_ensemble_classify`) against the
reference's numpy path on the same files.

Seeded synthetic members: K = 5 float16 probability files of one 180 x 512 x 512 case (crop box inside a 184 x 520 x 520 volume),
`c3` = 3 channels, `c15` = 15 channels.  The probabilities are a softmax of blocky logits plus voxel noise, so that, like stored
softmax files, most values are saturated and the files compress.  Per configuration:
  * the whole `merge_files(..., store_npz=True)` call (wall clock, one run);
  * its stages on their own: read + decompress the K members (one thread, and --threads threads), upload (host layout -> padded
    device layout), kernel (device events, median of --reps after a warm-up, mean kept and not kept), download + write (labels and
    mean to the host, the NIfTI, the compressed .npz of the mean);
  * the kernel against its minimum traffic, 2*K*C*V bytes read + V written (+ 2*C*V with the mean), and the bandwidth that gives;
  * with --host NAME[,NAME]: the reference's host leg on the same files, one run: np.load of every member, np.vstack, np.mean,
    argmax, insertion into the uncropped volume (read + decompress reported apart); labels and mean must equal the device's bit
    for bit, or the tool exits 1.
Reading and decompressing the files is host work on both sides and is reported separately, not hidden in a ratio.
One JSON line per configuration, all of them written to --out.

Run: python tools/bench_ensembling.py [--configs c3,c15] [--reps 20] [--host c3,c15] [--threads 5] [--workdir DIR]
     [--shape D,H,W] [--out profiles/ensembling_bench.json]"""
import argparse
import json
import os
import pickle
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, ROOT)

K = 5
SHAPE, FULL, LO = (180, 512, 512), (184, 520, 520), (2, 4, 4)
CONFIGS = {'c3': 3, 'c15': 15}
HBM_COPY_TBS = 6.29             # measured float4 copy of the chip (MI355X_MICROARCH.md), the yardstick of a pure stream


def _write_member(args):
    folder, C, seed = args
    rng = np.random.default_rng(seed)
    b = 4
    low = rng.standard_normal((C,) + tuple(s // b for s in SHAPE), dtype=np.float32) * 6
    out = np.empty((C,) + SHAPE, np.float16)
    for d in range(SHAPE[0]):
        lg = np.repeat(np.repeat(low[:, d // b], b, axis=1), b, axis=2)
        lg = lg + (rng.random(lg.shape[1:], dtype=np.float32) < 0.1) * rng.standard_normal(lg.shape, dtype=np.float32)
        e = np.exp(lg - lg.max(0))
        out[:, d] = e / e.sum(0)
    os.makedirs(folder, exist_ok=True)
    np.savez_compressed(os.path.join(folder, 'case.npz'), softmax=out)
    with open(os.path.join(folder, 'case.pkl'), 'wb') as f:
        pickle.dump({'size_after_cropping': np.array(SHAPE), 'original_size_of_raw_data': np.array(FULL),
                     'crop_bbox': [[LO[i], LO[i] + SHAPE[i]] for i in range(3)], 'itk_spacing': (0.8, 0.8, 2.5), 'itk_origin': (0., 0., 0.),
                     'itk_direction': tuple(np.eye(3).ravel()), 'original_spacing': np.array([2.5, 0.8, 0.8])}, f)
    return os.path.getsize(os.path.join(folder, 'case.npz'))


def _note(*a):
    print(*a, file=sys.stderr, flush=True)


def _load(f):
    return np.load(f)['softmax']


def bench(name, C, work, reps, threads, host):
    import torch
    from multitalent_amd.inference import ensemble_predictions as ep
    from multitalent_amd.utilities.nifti_io import write_image
    dev = torch.device('cuda', 0)
    V = int(np.prod(SHAPE))
    folders = [os.path.join(work, name, 'm%d' % k) for k in range(K)]
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        sizes = list(ex.map(_write_member, [(f, C, 100 * C + k) for k, f in enumerate(folders)]))
    res = {'config': name, 'members': K, 'channels': C, 'shape': list(SHAPE), 'voxels': V, 'member_bytes': 2 * C * V,
           'npz_bytes_per_member': int(np.mean(sizes)), 'generate_s': round(time.perf_counter() - t, 2)}
    _note(name, 'members written', res['generate_s'], 's')
    files, pkls = [os.path.join(f, 'case.npz') for f in folders], [os.path.join(f, 'case.pkl') for f in folders]
    out_file = os.path.join(work, name, 'out', 'case.nii.gz')
    os.makedirs(os.path.dirname(out_file))
    # warm-up of the runtime, the library and the kernel on a small problem
    small = [np.zeros((C, 4, 8, 8), np.float16)] * 2
    ep.merge_on_device(small, {'crop_bbox': None}, None, want_mean=True, device=dev)
    torch.cuda.synchronize()
    # ---- the whole call -------------------------------------------------------------------------------------------------------
    t = time.perf_counter()
    ep.merge_files(files, pkls, out_file, True, True)
    res['merge_files_s'] = round(time.perf_counter() - t, 3)
    _note(name, 'merge_files', res['merge_files_s'], 's')
    # ---- stages ---------------------------------------------------------------------------------------------------------------
    t = time.perf_counter()
    arrays = [_load(f) for f in files]
    res['read_decompress_1thread_s'] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        arrays = list(ex.map(_load, files))
    res['read_decompress_%dthreads_s' % threads] = round(time.perf_counter() - t, 3)
    torch.cuda.synchronize()
    t = time.perf_counter()
    members = [ep.upload_member(a, dev) for a in arrays]
    torch.cuda.synchronize()
    res['upload_s'] = round(time.perf_counter() - t, 3)
    cs = ep.padded_stride(V)
    out = torch.zeros(FULL, dtype=torch.uint8, device=dev)
    mean = torch.empty((C, cs), dtype=torch.float16, device=dev)
    for keep, key in ((True, 'kernel_mean_kept'), (False, 'kernel_labels_only')):
        times = []
        for r in range(reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ep.ensemble_classify(members, C, SHAPE, cs, out, LO, None, mean if keep else None, cs)
            e1.record()
            e1.synchronize()
            if r >= 3:
                times.append(e0.elapsed_time(e1) * 1e-3)
        med = float(np.median(times))
        traffic = 2 * K * C * V + V + (2 * C * V if keep else 0)
        res[key] = {'median_s': round(med, 6), 'min_s': round(min(times), 6), 'max_s': round(max(times), 6), 'reps': reps,
                    'min_traffic_bytes': traffic, 'TB_per_s': round(traffic / med / 1e12, 3),
                    'share_of_float4_copy': round(traffic / med / 1e12 / HBM_COPY_TBS, 3)}
    ep.ensemble_classify(members, C, SHAPE, cs, out, LO, None, mean, cs)
    torch.cuda.synchronize()
    t = time.perf_counter()
    seg = out.cpu().numpy()
    mean_np = mean[:, :V].cpu().numpy().reshape((C,) + SHAPE)
    res['download_s'] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    write_image(seg, out_file, (0.8, 0.8, 2.5))
    res['write_nifti_s'] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    np.savez_compressed(out_file[:-7] + '.npz', softmax=mean_np)
    res['write_npz_s'] = round(time.perf_counter() - t, 3)
    del members, mean, out
    _note(name, 'device stages done')
    ok = True
    if host:
        # the reference's leg (ensemble_predictions.py:28-30, segmentation_export.py:123-139) on the same files
        t = time.perf_counter()
        softmax = [np.load(f)['softmax'][None] for f in files]
        t_read = time.perf_counter() - t
        t = time.perf_counter()
        softmax = np.vstack(softmax)
        t_stack = time.perf_counter() - t
        t = time.perf_counter()
        m = np.mean(softmax, 0)
        t_mean = time.perf_counter() - t
        t = time.perf_counter()
        lab = m.argmax(0)
        full = np.zeros(FULL, dtype=np.uint8)
        full[LO[0]:LO[0] + SHAPE[0], LO[1]:LO[1] + SHAPE[1], LO[2]:LO[2] + SHAPE[2]] = lab
        t_dec = time.perf_counter() - t
        ok = bool(np.array_equal(full, seg) and np.array_equal(m.view(np.uint16), mean_np.view(np.uint16)))
        res['host'] = {'read_decompress_s': round(t_read, 3), 'vstack_s': round(t_stack, 3), 'mean_s': round(t_mean, 3),
                       'argmax_insert_s': round(t_dec, 3), 'compute_s': round(t_stack + t_mean + t_dec, 3), 'equals_device': ok}
    shutil.rmtree(os.path.join(work, name), ignore_errors=True)
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='c3,c15')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host', default='c3,c15')
    ap.add_argument('--threads', type=int, default=5)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--shape', default=None, help="D,H,W of the box instead of 180,512,512 (multiples of 4; for a quick check of the tool)")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ensembling_bench.json'))
    a = ap.parse_args()
    if a.shape:
        global SHAPE, FULL
        SHAPE = tuple(int(i) for i in a.shape.split(','))
        FULL = tuple(s + 8 for s in SHAPE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensembling needs a HIP device: there is no CPU fallback to time")
    work = tempfile.mkdtemp(prefix='mt_ens_bench_', dir=a.workdir)
    lines, good = [], True
    try:
        for name in a.configs.split(','):
            res, ok = bench(name, CONFIGS[name], work, a.reps, a.threads, name in a.host.split(','))
            good = good and ok
            print(json.dumps(res), flush=True)
            lines.append(res)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
    sys.exit(0 if good else 1)


if __name__ == '__main__':
    main()
