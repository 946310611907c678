"""Timing of the dataset fingerprint on the device (`DatasetAnalyzer.analyze_dataset`) against a host restatement of the reference's
algorithm with numpy.

Seeded synthetic folders of cropped cases, one CT modality with integer-valued HU and a blocky label map with 4 labels and a -1
border: `ct180` = 8 cases of 180 x 512 x 512, `cube128` = 64 cases of 128^3.  Per folder:
  * the whole `analyze_dataset()` call (wall clock: file reads, decompression, uploads, kernels, read-backs, pickles), median of
    --reps, and `analyse_segmentations()` once;
  * its stages on their own, summed over the cases: read and decompress the `.npz` files (one thread, and --threads threads),
    upload, sample (count + gather), select, moments;
  * each kernel with its minimum traffic and the bandwidth that gives: fg_sample_count (a read of the label map), fg_sample_gather
    (a second read, the samples read and written), select_kth_f32 on all samples of the folder (four reads), masked_moments (two
    reads), label_presence (a read of the label map);
  * with --host NAME[,NAME]: the reference's algorithm for those folders, one run: --threads worker processes that each read a
    case and return `list(modality[mask][::10])`, the lists concatenated, numpy's median / mean / std / min / max / percentile over
    the result and per case; the device's mn / mx must equal the host's and the other values agree to 1e-5 relative, or the tool
    exits 1.
The read and decompression of the files is host work on both sides and is reported separately, not hidden in a ratio.
One JSON line per folder, all of them written to --out.

Run: python tools/bench_dataset_analysis.py [--folders ct180,cube128] [--reps 3] [--host ct180] [--threads 16] [--workdir DIR]
     [--out profiles/dataset_analysis_bench.json]"""
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

FOLDERS = {'ct180': (8, (180, 512, 512)), 'cube128': (64, (128, 128, 128))}
KEYS = ('median', 'mean', 'sd', 'mn', 'mx', 'percentile_99_5', 'percentile_00_5')


def _write_case(args):
    folder, name, shape, seed = args
    rng = np.random.default_rng(seed)
    data = np.empty((2,) + shape, np.float32)
    for d in range(shape[0]):
        data[0, d] = np.clip(np.round(rng.standard_normal(shape[1:], dtype=np.float32) * 300 + 40), -1024, 3071)
    seg = data[1]
    seg[:] = 0
    for lab in range(1, 5):
        sz = [max(4, int(n / 2 * rng.uniform(0.5, 1.0))) for n in shape]
        lo = [int(rng.integers(0, n - s + 1)) for n, s in zip(shape, sz)]
        seg[lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = lab
    seg[:, :9, :] = -1
    seg[:, :, -11:] = -1
    np.savez_compressed(os.path.join(folder, name + '.npz'), data=data)
    with open(os.path.join(folder, name + '.pkl'), 'wb') as f:
        pickle.dump({'original_size_of_raw_data': np.array(shape) + 8, 'original_spacing': np.array([2.5, 0.8, 0.8]),
                     'size_after_cropping': shape}, f)


def make_folder(folder, name, threads):
    ncases, shape = FOLDERS[name]
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, 'dataset.json'), 'w') as f:
        json.dump({'modality': {'0': 'CT'}, 'labels': {str(i): 'l%d' % i for i in range(5)}}, f)
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(_write_case, [(folder, 'case_%03d' % i, shape, i) for i in range(ncases)]))


def timed(fn, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _host_voxels(args):
    folder, name, mod = args
    a = np.load(os.path.join(folder, name + '.npz'))['data']
    return list(a[mod][a[-1] > 0][::10])


def _host_stats(voxels):
    if len(voxels) == 0:
        return (np.nan,) * 7
    return (np.median(voxels), np.mean(voxels), np.std(voxels), np.min(voxels), np.max(voxels), np.percentile(voxels, 99.5),
            np.percentile(voxels, 0.5))


def host_leg(folder, names, threads):
    import multiprocessing
    t0 = time.perf_counter()
    with multiprocessing.get_context('spawn').Pool(threads) as p:      # fresh workers: none of them holds the device
        v = p.map(_host_voxels, [(folder, n, 0) for n in names])
        t_read = time.perf_counter() - t0
        w = []
        for iv in v:
            w += iv
        glob = _host_stats(w)
        local = p.map(_host_stats, v)
    return glob, local, time.perf_counter() - t0, t_read


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--folders', default='ct180,cube128')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host', default='')
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--workdir', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from multitalent_amd import ops
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer, _stat_ranks
    work = tempfile.mkdtemp(prefix='dataset_analysis_bench_', dir=a.workdir)
    lines, ok = [], True
    try:
        for name in a.folders.split(','):
            folder = os.path.join(work, name)
            t0 = time.perf_counter()
            make_folder(folder, name, a.threads)
            t_make = time.perf_counter() - t0
            an = DatasetAnalyzer(folder, num_processes=a.threads)
            walls = []
            for it in range(a.reps + 1):                             # the first call is the warm-up
                t0 = time.perf_counter()
                dp = an.analyze_dataset()
                torch.cuda.synchronize()
                if it:
                    walls.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            an.analyse_segmentations()
            t_seg = time.perf_counter() - t0
            ids = an.patient_identifiers
            # stages
            t0 = time.perf_counter()
            arrays = [an._load_case(p) for p in ids[:min(len(ids), 8)]]
            t_read1 = (time.perf_counter() - t0) * len(ids) / len(arrays)
            del arrays
            t0 = time.perf_counter()
            with ThreadPoolExecutor(max_workers=a.threads) as pool:
                for arr in pool.map(an._load_case, ids):
                    del arr
            t_readn = time.perf_counter() - t0
            st = {k: 0.0 for k in ('upload', 'count', 'gather', 'select_per_case', 'moments_per_case', 'label_presence')}
            V_total = fg_total = m_total = 0
            chunks = []
            for p in ids:
                host = np.ascontiguousarray(an._load_case(p), dtype=np.float32)
                vol, ms = timed(lambda: torch.from_numpy(host).cuda().reshape(host.shape[0], -1), torch)
                st['upload'] += ms
                data, seg = vol[:1], vol[-1]
                ops.fg_sample_count(seg)                             # warm
                index, ms = timed(lambda: ops.fg_sample_count(seg), torch)
                st['count'] += ms
                (samples, n, _), ms = timed(lambda: ops.fg_sample(data, seg, 10, index=index), torch)
                st['gather'] += ms
                _, ms = timed(lambda: ops.label_presence(seg), torch)
                st['label_presence'] += ms
                if samples.shape[1]:
                    _, ms = timed(lambda: ops.select_kth_f32(samples[0], _stat_ranks(samples.shape[1])), torch)
                    st['select_per_case'] += ms
                    _, ms = timed(lambda: ops.masked_moments(samples, ops.MOMENTS_ALL), torch)
                    st['moments_per_case'] += ms
                chunks.append(samples[0].clone())
                V_total += seg.numel(); fg_total += n; m_total += samples.shape[1]
                del vol, data, seg, samples, index
            allv = torch.cat(chunks)
            del chunks
            ranks = _stat_ranks(allv.numel())
            ops.select_kth_f32(allv, ranks)
            _, ms_sel = timed(lambda: ops.select_kth_f32(allv, ranks), torch)
            _, ms_mom = timed(lambda: ops.masked_moments(allv[None], ops.MOMENTS_ALL), torch)
            traffic = {'fg_sample_count': 4 * V_total, 'fg_sample_gather': 4 * V_total + 8 * m_total,
                       'label_presence': 4 * V_total, 'select_kth_f32_all_samples': 16 * m_total, 'masked_moments_all_samples': 8 * m_total}
            kern_ms = {'fg_sample_count': st['count'], 'fg_sample_gather': st['gather'], 'label_presence': st['label_presence'],
                       'select_kth_f32_all_samples': ms_sel, 'masked_moments_all_samples': ms_mom}
            res = {'metric': 'analyze_dataset %s: %d cases of %s, 1 modality' % (name, len(ids), 'x'.join(str(i) for i in FOLDERS[name][1])),
                   'analyze_dataset_wall_s_median': float(np.median(walls)), 'reps': a.reps, 'analyse_segmentations_wall_s': t_seg,
                   'threads': a.threads, 'make_folder_s': t_make,
                   'read_decompress_s': {'one_thread': t_read1, 'threads': t_readn},
                   'stage_ms': {'upload': st['upload'], 'sample': st['count'] + st['gather'],
                                'select': st['select_per_case'] + ms_sel, 'moments': st['moments_per_case'] + ms_mom},
                   'kernel_ms': kern_ms, 'kernel_min_bytes': traffic,
                   'kernel_gb_per_s': {k: traffic[k] / (kern_ms[k] * 1e-3) / 1e9 for k in kern_ms if kern_ms[k] > 0},
                   'voxels': V_total, 'foreground_voxels': fg_total, 'samples': m_total}
            if name in a.host.split(','):
                glob, local, t_host, t_host_read = host_leg(folder, ids, a.threads)
                res['host_s'] = t_host
                res['host_read_and_sample_s'] = t_host_read
                res['host_statistics_s'] = t_host - t_host_read
                ip = dp['intensityproperties'][0]
                rows = [(ip, glob)] + [(ip['local_props'][p], local[i]) for i, p in enumerate(ids)]
                worst = 0.0
                same = True
                for got, want in rows:
                    for k, w in zip(KEYS, want):
                        if k in ('mn', 'mx'):
                            same = same and got[k] == w
                        else:
                            worst = max(worst, abs(float(got[k]) - float(w)) / max(1.0, abs(float(w))))
                res['max_relative_difference'] = worst
                res['consistent'] = bool(same and worst <= 1e-5)
                ok = ok and res['consistent']
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
            del allv
            torch.cuda.empty_cache()
            shutil.rmtree(folder)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
