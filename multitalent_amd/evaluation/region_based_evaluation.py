"""Region-based evaluation (reference evaluation/region_based_evaluation.py:12-110): Dice per region - a region is the union of
its labels, such as KiTS' "kidney incl tumor" = (1, 2) - for every predicted case of a folder, written to `summary.csv` with the
reference's layout and number format.

One case is one upload of the pair (`.nii.gz` files are inflated on the device, evaluator._load) and ONE joint label histogram
for all regions (evaluator._device_counts); a region's tp / fp / fn are sums of its cells.  Without a HIP device, or for volumes
that are not integer labels in 0..255, the evaluator's host loop counts instead: the same integers, the same csv.

With `nsd_threshold` (mm: one number or {region name: number}) a second table `summary_nsd.csv` of the normalized surface Dice
(evaluator.NSD_METRIC, HIP device only) is written in the same layout; without it nothing extra runs.

Run: python -m multitalent_amd.evaluation.region_based_evaluation -pred DIR -ref DIR --regions kits|brats|FILE.json [--nsd TOL]"""
import json
import os
import warnings

import numpy as np

from . import evaluator as E


def get_brats_regions():
    """Valid for BraTS data relabelled to 1, 2, 3 (the convention of the reference's Task conversion), not for the original labels."""
    return {"whole tumor": (1, 2, 3), "tumor core": (2, 3), "enhancing tumor": (3,)}


def get_KiTS_regions():
    return {"kidney incl tumor": (1, 2), "tumor": (2,)}


def create_region_from_mask(mask, join_labels):
    """mask: label volume, a device tensor (or a numpy array); -> uint8 volume of the same kind, 1 where the label is one of
    join_labels.  The scoring below does not call it: it reads every region from one histogram."""
    try:
        import torch
        if torch.is_tensor(mask):
            out = torch.zeros_like(mask, dtype=torch.uint8)
            for l in join_labels:
                out[mask == l] = 1
            return out
    except ImportError:
        pass
    return np.isin(np.asarray(mask), list(join_labels)).astype(np.uint8)


def dice_from_counts(tp, fp, fn):
    """NaN when both masks are empty (region_based_evaluation.py:48), else medpy's dc: 2 * intersection / (|pred| + |gt|) in that
    order - 0.0 when only one of them is empty."""
    tp, fp, fn = int(tp), int(fp), int(fn)
    size_pred, size_gt = tp + fp, tp + fn
    if size_pred == 0 and size_gt == 0:
        return float("NaN")
    return 2. * tp / float(size_pred + size_gt)


def _region_counts(test, ref, regions):
    """[(tp, fp, fn, tn)] per region of the loaded pair: one joint histogram on the device, else the host loop."""
    if tuple(test.shape) != tuple(ref.shape):
        raise ValueError("Shape mismatch: %s and %s" % (tuple(test.shape), tuple(ref.shape)))
    pair = E._device_pair(test, ref)
    if pair is not None:
        counts = E._device_counts(pair[0], pair[1], regions)
        return pair, [counts[str(r)] for r in regions]
    if E._is_device_tensor(test):
        test = test.cpu().numpy()
    if E._is_device_tensor(ref):
        ref = ref.cpu().numpy()
    out = []
    for r in regions:
        t, g = np.isin(test, list(r)), np.isin(ref, list(r))
        tp, fp, fn = int((t & g).sum()), int((t & ~g).sum()), int((~t & g).sum())
        out.append((tp, fp, fn, int(t.size) - tp - fp - fn))
    return None, out


def _evaluate_case(file_pred, file_gt, regions, tolerances=None, connectivity=1):
    """-> (Dice per region, NSD per region or None).  tolerances: one number per region, or None."""
    regions = [tuple(r) for r in regions]
    test, _, spacing = E._load(file_pred)
    ref, _, _ = E._load(file_gt)
    pair, counts = _region_counts(test, ref, regions)
    dice = [dice_from_counts(tp, fp, fn) for tp, fp, fn, _ in counts]
    if tolerances is None:
        return dice, None
    if pair is None:
        import torch
        if not torch.cuda.is_available():
            E._no_device()
        raise ValueError("the normalized surface Dice needs integer label volumes with values in 0..255")
    if len(tuple(test.shape)) != 3:
        raise ValueError("the normalized surface Dice needs 3-D volumes [z, y, x], got shape %s" % (tuple(test.shape),))
    sp = None if spacing is None else np.array(spacing, dtype=np.float64)[::-1]         # the prediction's, (z, y, x)
    nsd = [E._surface_metrics(pair[0], pair[1], r, c, [E.NSD_METRIC], sp, connectivity, tol)[E.NSD_METRIC]
           for r, c, tol in zip(regions, counts, tolerances)]
    return dice, nsd


def evaluate_case(file_pred, file_gt, regions):
    """file names (or arrays / device tensors), regions: iterable of label tuples -> [Dice per region]"""
    return _evaluate_case(file_pred, file_gt, regions)[0]


def write_summary_csv(fname, case_names, region_names, results):
    """results[i][k]: the value of region k for case i (NaN allowed).  The reference's table: header, one row per case, then
    mean, median, and both again with NaN counted as 1; every number as %02.4f."""
    cols = [[float(results[i][k]) for i in range(len(case_names))] for k in range(len(region_names))]

    def row(name, values):
        return name + "".join(",%02.4f" % v for v in values) + "\n"

    def nan_is_1(c):
        c = np.array(c, dtype=np.float64)
        c[np.isnan(c)] = 1
        return c
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # a column of NaN only: nan, as in the reference
        with np.errstate(all='ignore'):
            lines = ["casename" + "".join(",%s" % r for r in region_names) + "\n"]
            for i, name in enumerate(case_names):
                lines.append(row(name, [c[i] for c in cols]))
            lines.append(row("mean", [np.nanmean(c) for c in cols]))
            lines.append(row("median", [np.nanmedian(c) for c in cols]))
            lines.append(row("mean (nan is 1)", [np.mean(nan_is_1(c)) for c in cols]))
            lines.append(row("median (nan is 1)", [np.median(nan_is_1(c)) for c in cols]))
    with open(fname, 'w') as f:
        f.write("".join(lines))


def _region_tolerances(regions, nsd_threshold):
    """one tolerance per region from a number or a dict {region name: number}"""
    if nsd_threshold is None:
        return None
    labels = list(regions.keys())
    by_name = E._nsd_tolerances(labels, nsd_threshold)
    return [by_name[str(n)] for n in labels]


def evaluate_regions(folder_predicted, folder_gt, regions, processes=None, nsd_threshold=None, connectivity=1):
    """Every .nii.gz of folder_predicted against the file of the same name in folder_gt -> folder_predicted/summary.csv (and
    summary_nsd.csv with nsd_threshold).  A prediction without ground truth is an AssertionError, a ground truth without prediction
    a printed warning.  `processes` is accepted for the reference's callers and not used: the cases run one after another on the
    device."""
    region_names = list(regions.keys())
    tolerances = _region_tolerances(regions, nsd_threshold)

    def niftis(folder):
        return sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(".nii.gz"))
    files_in_pred, files_in_gt = niftis(folder_predicted), niftis(folder_gt)
    have_no_gt = [i for i in files_in_pred if i not in files_in_gt]
    assert len(have_no_gt) == 0, "Some files in folder_predicted have not ground truth in folder_gt"
    if any(i not in files_in_pred for i in files_in_gt):
        print("WARNING! Some files in folder_gt were not predicted (not present in folder_predicted)!")
    dice, nsd = [], []
    for i in files_in_pred:
        d, n = _evaluate_case(os.path.join(folder_predicted, i), os.path.join(folder_gt, i), list(regions.values()), tolerances,
                              connectivity)
        dice.append(d)
        nsd.append(n)
    case_names = [i[:-7] for i in files_in_pred]
    write_summary_csv(os.path.join(folder_predicted, 'summary.csv'), case_names, region_names, dice)
    if tolerances is not None:
        write_summary_csv(os.path.join(folder_predicted, 'summary_nsd.csv'), case_names, region_names, nsd)


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description="Dice per region for every case of a folder of predictions -> summary.csv there")
    parser.add_argument('-pred', required=True, type=str, help="Folder with the predicted segmentations (.nii.gz).")
    parser.add_argument('-ref', required=True, type=str, help="Folder with the ground truth; the file names must match.")
    parser.add_argument('--regions', required=True, type=str,
                        help="kits, brats, or a json file {region name: [labels]} (the order of the file is the column order).")
    parser.add_argument('--nsd', type=float, default=None, metavar='TOL',
                        help="Also summary_nsd.csv: %r at this tolerance in mm (HIP device only)." % E.NSD_METRIC)
    args = parser.parse_args(argv)
    if args.regions == 'kits':
        regions = get_KiTS_regions()
    elif args.regions == 'brats':
        regions = get_brats_regions()
    else:
        with open(args.regions) as f:
            regions = {k: tuple(int(i) for i in v) for k, v in json.load(f).items()}
    return evaluate_regions(args.pred, args.ref, regions, nsd_threshold=args.nsd)


if __name__ == '__main__':
    main()
