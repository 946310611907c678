"""Timing of the device evaluation against the host path.

The seeded 512^3 label volume of tools/bench_postprocessing.py (`make_volume`: three organ-like blobs, a few hundred spurious
blobs and a percolation slab, so every label has millions of border voxels) is the prediction; the same volume shifted by
(3, -2, 4) voxels is the ground truth.  Labels [1, 2, 3] plus the tuple (1, 2, 3).  On device tensors, with device events, after a
warm-up, median of --reps:
  * `evaluate_case` with the default metrics (one joint-histogram launch for all labels),
  * `evaluate_case(advanced=True)` with all four surface-distance metrics (spacing (2.5, 0.8, 0.8)).
Against that the host leg on the same volume: the evaluator's numpy loop (np.isin + boolean reductions per label) and, for the
surface part, the scipy restatement of medpy's algorithm in tests/evaluation_cases.py (--no-host skips both, --no-host-surface
the scipy part: it takes minutes at 512^3).  Device and host must agree within the bounds of tests/test_evaluation_gpu.py
(default metrics ==, hd / hd95 relative 1e-12, asd / assd 1e-10) or the tool exits 1.  The algorithmic bytes and the HBM-bound
time from them are printed with the measured times as one JSON line (and written to --out).

--nsd TOL adds the normalized surface Dice at TOL mm to the same run:
  * `evaluate_case(advanced=True)` with the four metrics, without and with "Normalized Surface Dice", ALTERNATING, median of --reps
    after a warm-up pair, device events: what the extra launch and read-back per entry cost inside the call;
  * the count kernel alone (`ops.sd_count_within` on each entry's distance array, --kernel-reps launches between two events) against
    8 bytes per border voxel at the streaming figure;
  * on the host leg the same count with numpy on the scipy distances (the distances are the expensive part and are shared with
    the four metrics: both times are reported); device and host values must agree to 1e-12 or the tool exits 1.

Run: python tools/bench_evaluation.py [--size 512] [--reps 5] [--nsd TOL] [--no-host | --no-host-surface] [--out FILE]
Kernel statistics: rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_evaluation.py --no-host --reps 3"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from bench_postprocessing import HBM_BYTES_PER_S, make_volume  # noqa: E402

LABELS = [1, 2, 3, (1, 2, 3)]
SPACING = (2.5, 0.8, 0.8)
ADVANCED = ["Hausdorff Distance", "Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance"]
NSD = "Normalized Surface Dice"
NSD_BYTES_PER_BORDER_VOXEL = 8                                  # the count reads every distance once and nothing else
# joint histogram: both volumes read once, for all labels
HIST_BYTES_PER_VOXEL = 2
# surface distances, per voxel and label entry: border (both volumes read, border byte written; neighbour reads hit the cache),
# compaction (border byte read), rows (border byte read, 2 x int16 written)
SD_BYTES_PER_VOXEL_PER_ENTRY = {'border': 3, 'compact': 1, 'rows': 5}
# per border voxel: index written and read (8), distance written, read by the reduction and by 8 select passes (80); the row
# candidates the query reads depend on the data and are not counted
SD_BYTES_PER_BORDER_VOXEL = 88


def shifted(img, shift=(3, -2, 4)):
    out = np.zeros_like(img)
    src = tuple(slice(max(0, -s), img.shape[i] - max(0, s)) for i, s in enumerate(shift))
    dst = tuple(slice(max(0, s), img.shape[i] - max(0, -s)) for i, s in enumerate(shift))
    out[dst] = img[src]
    return out


def timed(fn, reps):
    import torch
    times, res = [], None
    for it in range(reps + 1):                                  # the first call is the warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            times.append(e0.elapsed_time(e1))
    return res, float(np.median(times)), float(np.min(times))


def timed_alternating(fns, reps):
    """fns called in turn, reps + 1 rounds (the first is the warm-up) -> per fn (last result, median ms, min ms), device events"""
    import torch
    times, res = [[] for _ in fns], [None] * len(fns)
    for it in range(reps + 1):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res[k] = fn()
            e1.record()
            torch.cuda.synchronize()
            if it:
                times[k].append(e0.elapsed_time(e1))
    return [(res[k], float(np.median(times[k])), float(np.min(times[k]))) for k in range(len(fns))]


def nsd_device(t, r, pred, gt, tol, reps, kernel_reps):
    """The --nsd measurements on the device -> (dict for the result line, evaluate_case's result with NSD)"""
    import torch
    from multitalent_amd import ops
    from multitalent_amd.evaluation.evaluator import evaluate_case
    kw = dict(advanced=True, voxel_spacing=SPACING)
    (_, off_ms, off_min), (with_nsd, on_ms, on_min) = timed_alternating(
        [lambda: evaluate_case(t, r, LABELS, advanced_metrics=ADVANCED, **kw),
         lambda: evaluate_case(t, r, LABELS, advanced_metrics=ADVANCED + [NSD], nsd_threshold=tol, **kw)], reps)
    kernel_ms, borders = [], []
    for l in LABELS:
        members = list(l) if isinstance(l, tuple) else [l]
        member = np.zeros(256, bool)
        member[members] = True
        cap = int(np.isin(pred, members).sum() + np.isin(gt, members).sum())
        sds, stats = ops.surface_distances(t, r, member, SPACING, 1, capacity=cap)
        st = stats.cpu().numpy()
        n_tr, n_rt = int(st[0]), int(st[3])
        out = torch.empty((2, 1), dtype=torch.int64, device=t.device)
        ops.sd_count_within(sds, n_tr, n_rt, [tol], out=out)                # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(kernel_reps):
            ops.sd_count_within(sds, n_tr, n_rt, [tol], out=out)
        e1.record()
        torch.cuda.synchronize()
        kernel_ms.append(e0.elapsed_time(e1) / kernel_reps)
        borders.append(n_tr + n_rt)
    bound_ms = [NSD_BYTES_PER_BORDER_VOXEL * b / HBM_BYTES_PER_S * 1e3 for b in borders]
    res = {'nsd_tolerance_mm': tol, 'advanced_without_nsd_ms_median': off_ms, 'advanced_without_nsd_ms_min': off_min,
           'advanced_with_nsd_ms_median': on_ms, 'advanced_with_nsd_ms_min': on_min, 'nsd_part_device_ms': on_ms - off_ms,
           'nsd_part_device_ms_per_entry': (on_ms - off_ms) / len(LABELS), 'nsd_kernel_reps': kernel_reps,
           'nsd_kernel_ms_per_entry': kernel_ms, 'nsd_border_voxels_per_entry': borders,
           'nsd_bytes_per_border_voxel': NSD_BYTES_PER_BORDER_VOXEL, 'nsd_kernel_hbm_bound_ms_per_entry': bound_ms,
           'nsd_kernel_share_of_hbm_bound': sum(bound_ms) / sum(kernel_ms),
           'nsd_values': {str(l): with_nsd[str(l)][NSD] for l in LABELS}}
    return res, with_nsd


def nsd_numpy(a_to_b, b_to_a, threshold):
    """the reference's arithmetic (evaluation/surface_dice.py:46-55 there) on two arrays of distances"""
    tp_a = np.sum(a_to_b <= threshold) / len(a_to_b)
    tp_b = np.sum(b_to_a <= threshold) / len(b_to_a)
    fp = np.sum(a_to_b > threshold) / len(a_to_b)
    fn = np.sum(b_to_a > threshold) / len(b_to_a)
    return float((tp_a + tp_b) / (tp_a + tp_b + fp + fn + 1e-8))


def rel(a, b):
    if math.isnan(a) and math.isnan(b) or a == b:
        return 0.0
    return abs(a - b) / abs(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--no-host-surface', action='store_true')
    ap.add_argument('--nsd', type=float, default=None, metavar='TOL', help="also the normalized surface Dice at TOL mm")
    ap.add_argument('--kernel-reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from multitalent_amd.evaluation.evaluator import confusion_metrics, evaluate_case
    n = a.size
    pred = make_volume(n)
    gt = shifted(pred)
    t, r = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    dflt, dflt_ms, dflt_min = timed(lambda: evaluate_case(t, r, LABELS), a.reps)
    adv, adv_ms, adv_min = timed(lambda: evaluate_case(t, r, LABELS, advanced=True, advanced_metrics=ADVANCED, voxel_spacing=SPACING),
                                 a.reps)
    V = n ** 3
    hist_bound_ms = HIST_BYTES_PER_VOXEL * V / HBM_BYTES_PER_S * 1e3
    from multitalent_amd import ops
    borders = 0
    for l in LABELS:                                            # border voxels per entry, for the byte count
        member = np.zeros(256, bool)
        member[list(l) if isinstance(l, tuple) else [l]] = True
        cap = int(np.isin(pred, np.flatnonzero(member)).sum() + np.isin(gt, np.flatnonzero(member)).sum())
        st = ops.surface_distances(t, r, member, SPACING, 1, capacity=cap)[1].cpu().numpy()
        borders += int(st[0] + st[3])
    sd_bytes = sum(SD_BYTES_PER_VOXEL_PER_ENTRY.values()) * V * len(LABELS) + SD_BYTES_PER_BORDER_VOXEL * borders
    sd_bound_ms = sd_bytes / HBM_BYTES_PER_S * 1e3
    surface_ms = adv_ms - dflt_ms
    res = {'metric': 'evaluate_case %d^3, labels %s' % (n, LABELS), 'reps': a.reps,
           'default_device_ms_median': dflt_ms, 'default_device_ms_min': dflt_min,
           'advanced_device_ms_median': adv_ms, 'advanced_device_ms_min': adv_min, 'surface_part_device_ms': surface_ms,
           'hist_algorithmic_bytes': HIST_BYTES_PER_VOXEL * V, 'hist_hbm_bound_ms': hist_bound_ms,
           'hist_share_of_hbm_bound': hist_bound_ms / dflt_ms,
           'surface_algorithmic_bytes': sd_bytes, 'surface_bytes_per_voxel_per_entry': SD_BYTES_PER_VOXEL_PER_ENTRY,
           'surface_bytes_per_border_voxel': SD_BYTES_PER_BORDER_VOXEL, 'border_voxels_all_entries': borders,
           'surface_hbm_bound_ms': sd_bound_ms, 'surface_share_of_hbm_bound': sd_bound_ms / surface_ms}
    ok = True
    with_nsd = None
    if a.nsd is not None:
        nsd_res, with_nsd = nsd_device(t, r, pred, gt, a.nsd, a.reps, a.kernel_reps)
        res.update(nsd_res)
    if not a.no_host:
        t0 = time.perf_counter()
        host = {}
        for l in LABELS:
            members = list(l) if isinstance(l, tuple) else [l]
            host[str(l)] = confusion_metrics(np.isin(pred, members), np.isin(gt, members))
        res['default_host_numpy_s'] = time.perf_counter() - t0
        for l in LABELS:
            for k, v in host[str(l)].items():
                same = (math.isnan(v) and math.isnan(dflt[str(l)][k])) or v == dflt[str(l)][k]
                ok = ok and same and adv[str(l)][k] == dflt[str(l)][k]
        res['default_identical'] = bool(ok)
        if not a.no_host_surface:
            import evaluation_cases as EC
            t0 = time.perf_counter()
            worst_hd, worst_mean, worst_nsd, nsd_count_s = 0.0, 0.0, 0.0, 0.0
            for l in LABELS:
                members = list(l) if isinstance(l, tuple) else [l]
                A, B = np.isin(pred, members), np.isin(gt, members)
                s1 = EC.surface_distances_scipy(A, B, SPACING, 1)
                s2 = EC.surface_distances_scipy(B, A, SPACING, 1)
                want = {"Hausdorff Distance": max(s1.max(), s2.max()), "Hausdorff Distance 95": np.percentile(np.hstack((s1, s2)), 95),
                        "Avg. Surface Distance": s1.mean(), "Avg. Symmetric Surface Distance": np.mean((s1.mean(), s2.mean()))}
                for k, v in want.items():
                    e = rel(adv[str(l)][k], float(v))
                    if k.startswith("Hausdorff"):
                        worst_hd = max(worst_hd, e)
                    else:
                        worst_mean = max(worst_mean, e)
                if with_nsd is not None:
                    t1 = time.perf_counter()
                    v = nsd_numpy(s1, s2, a.nsd)
                    nsd_count_s += time.perf_counter() - t1
                    worst_nsd = max(worst_nsd, abs(with_nsd[str(l)][NSD] - v))
            res['surface_host_scipy_s'] = time.perf_counter() - t0
            if with_nsd is not None:
                # the host's NSD needs the same two scipy distance arrays per entry: all of surface_host_scipy_s but the few
                # seconds of the four metrics' own reductions, of which nsd_host_count_s is the counting alone
                res['nsd_host_count_s'], res['worst_abs_nsd'] = nsd_count_s, worst_nsd
                ok = ok and worst_nsd <= 1e-12
            res['worst_rel_hd_hd95'], res['worst_rel_asd_assd'] = worst_hd, worst_mean
            ok = ok and worst_hd <= 1e-12 and worst_mean <= 1e-10
    res['agree'] = bool(ok)
    res['advanced_values'] = {str(l): {k: adv[str(l)][k] for k in ADVANCED} for l in LABELS}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
