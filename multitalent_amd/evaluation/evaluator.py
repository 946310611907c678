"""`aggregate_scores` as `trainer.validate()` calls it, `evaluate_folder` and the command line of `nnunet_evaluate_folder`
(reference evaluation/evaluator.py:30-56,152-225,297-400,446-483 with the metrics of evaluation/metrics.py:105-383): per case and
label the thirteen default metrics, with `advanced=True` the surface-distance metrics behind them, their nan-mean over the cases,
and the reference's summary.json layout.

With a HIP device the confusion counts of ALL labels of a case come from one joint label histogram of the once-uploaded pair
(`mt_seg_joint_hist`); without one, or for volumes that are not integer labels in 0..255, the host loop below counts them.  Both
feed `metrics_from_counts`, so the default metrics are the same numbers bit for bit.  The advanced metrics (medpy's hd, hd95,
asd, assd: borders by erosion, exact Euclidean distance transform, `mt_surface_distances` / `mt_select_kth`) exist on the device
only: without one they raise.  So does "Normalized Surface Dice" at `nsd_threshold` mm (reference evaluation/surface_dice.py): the
same distances counted against the tolerance where they lie (`mt_sd_count_within`), two integers per label entry read back.

Run: python -m multitalent_amd.evaluation.evaluator -ref GT_FOLDER -pred PRED_FOLDER -l 1 2 3 [--advanced] [--nsd TOL_MM]"""
import hashlib
import json
from collections import OrderedDict
from datetime import datetime

import numpy as np

from ..utilities.nifti_io import read_image, read_image_device

DEFAULT_METRICS = ["False Positive Rate", "Dice", "Jaccard", "Precision", "Recall", "Accuracy", "False Omission Rate",
                   "Negative Predictive Value", "False Negative Rate", "True Negative Rate", "False Discovery Rate",
                   "Total Positives Test", "Total Positives Reference"]


ADVANCED_METRICS = ["Hausdorff Distance", "Hausdorff Distance 95", "Avg. Surface Distance", "Avg. Symmetric Surface Distance"]
DEFAULT_ADVANCED_METRICS = ["Hausdorff Distance 95"]          # Evaluator.default_advanced_metrics (evaluator.py:53-58)
NSD_METRIC = "Normalized Surface Dice"                        # accepted in `advanced_metrics` beside ADVANCED_METRICS, with nsd_threshold


def metrics_from_counts(tp, fp, fn, tn):
    """Confusion counts of one label (Python ints) -> OrderedDict of DEFAULT_METRICS (NaN where the reference returns NaN)."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    test_empty, test_full = (tp + fp) == 0, (tn + fn) == 0
    ref_empty, ref_full = (tp + fn) == 0, (tn + fp) == 0
    nan = float("NaN")
    spec = nan if ref_full else tn / (tn + fp)
    prec = nan if test_empty else tp / (tp + fp)
    sens = nan if ref_empty else tp / (tp + fn)
    fom = nan if test_full else fn / (fn + tn)
    both_empty = test_empty and ref_empty
    m = OrderedDict()
    m["False Positive Rate"] = 1 - spec
    m["Dice"] = nan if both_empty else 2. * tp / (2 * tp + fp + fn)
    m["Jaccard"] = nan if both_empty else tp / (tp + fp + fn)
    m["Precision"] = prec
    m["Recall"] = sens
    m["Accuracy"] = (tp + tn) / (tp + fp + tn + fn)
    m["False Omission Rate"] = fom
    m["Negative Predictive Value"] = 1 - fom
    m["False Negative Rate"] = 1 - sens
    m["True Negative Rate"] = spec
    m["False Discovery Rate"] = 1 - prec
    m["Total Positives Test"] = tp + fp
    m["Total Positives Reference"] = tp + fn
    return OrderedDict((k, float(v)) for k, v in m.items())


def confusion_metrics(test, reference):
    """test / reference: boolean masks of one label -> OrderedDict of DEFAULT_METRICS (NaN where the reference returns NaN)."""
    tp = int((test & reference).sum())
    fp = int((test & ~reference).sum())
    fn = int((~test & reference).sum())
    tn = int(test.size) - tp - fp - fn
    return metrics_from_counts(tp, fp, fn, tn)


def nsd_from_counts(c_tr, n_tr, c_rt, n_rt):
    """surface_dice.py:46-55 on integers: n_tr / n_rt border voxels of test / reference, c_tr / c_rt of them within the tolerance
    of the other border.  Python's float arithmetic on ints below 2^53 is numpy's float64 arithmetic: the same bits."""
    c_tr, n_tr, c_rt, n_rt = int(c_tr), int(n_tr), int(c_rt), int(n_rt)
    tp_a = c_tr / n_tr
    tp_b = c_rt / n_rt
    fp = (n_tr - c_tr) / n_tr
    fn = (n_rt - c_rt) / n_rt
    return (tp_a + tp_b) / (tp_a + tp_b + fp + fn + 1e-8)


def _nsd_tolerances(labels, nsd_threshold):
    """{str(label): tolerance in mm} from a number for all entries or a dict {str(label): number}; an entry without one, or a
    tolerance that is not a number >= 0, is a ValueError."""
    out = OrderedDict()
    for l in labels:
        v = nsd_threshold.get(str(l)) if isinstance(nsd_threshold, dict) else nsd_threshold
        if v is None:
            raise ValueError("%r needs nsd_threshold: a tolerance in mm, or a dict {str(label): mm} with an entry for label %s"
                             % (NSD_METRIC, l))
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError("nsd_threshold for label %s must be a number, got %r" % (l, v))
        if not v >= 0:                                          # False for NaN
            raise ValueError("nsd_threshold for label %s must be >= 0, got %r" % (l, v))
        out[str(l)] = v
    return out


def _no_device():
    raise RuntimeError("multitalent_amd: the surface-distance (advanced) metrics run on a HIP device only; there is no CPU fallback")


def _members(l):
    return tuple(l) if isinstance(l, (tuple, list)) else (l,)


def _is_device_tensor(x):
    import torch
    return torch.is_tensor(x) and x.is_cuda


def _device_uint8(x, dev):
    """-> contiguous uint8 tensor on dev holding x, or None when x is not an integer volume with values in 0..255."""
    import torch
    if torch.is_tensor(x):
        if x.dtype != torch.uint8:
            if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
                return None
            if x.numel() and (int(x.min()) < 0 or int(x.max()) > 255):
                return None
        return x.to(device=dev, dtype=torch.uint8).contiguous()
    if x.dtype != np.uint8:
        if x.dtype.kind not in 'iu':
            return None
        if x.size and (int(x.min()) < 0 or int(x.max()) > 255):
            return None
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8)).to(dev)


def _device_pair(test, ref):
    """The pair as uint8 device tensors when a HIP device is there and both volumes are integer labels in 0..255, else None."""
    import torch
    if _is_device_tensor(test):
        dev = test.device
    elif _is_device_tensor(ref):
        dev = ref.device
    elif torch.cuda.is_available():
        dev = torch.device('cuda', torch.cuda.current_device())
    else:
        return None
    if int(np.prod(tuple(test.shape), dtype=np.int64)) == 0:
        return None
    with torch.cuda.device(dev):
        t = _device_uint8(test, dev)
        r = _device_uint8(ref, dev) if t is not None else None
    return None if t is None or r is None else (t, r)


def _device_counts(t, r, labels):
    """{str(label): (tp, fp, fn, tn)} of every label entry from one joint histogram.  Every distinct member value gets a class
    of its own, all other values share class 0; an entry's counts are sums of cells."""
    from .. import ops
    values = sorted({int(m) for l in labels for m in _members(l) if 0 <= int(m) <= 255})
    first = 1 if len(values) < 256 else 0                       # class 0 = "every other value" while there is one
    cls = {v: i + first for i, v in enumerate(values)}
    remap = np.zeros(256, dtype=np.uint8)
    for v, c in cls.items():
        remap[v] = c
    ncls = len(values) + first
    import torch
    with torch.cuda.device(t.device):
        hist = ops.seg_joint_hist(t, r, remap, ncls).cpu().numpy()
    total = int(t.numel())
    counts = OrderedDict()
    for l in labels:
        sel = np.zeros(ncls, dtype=bool)
        for m in _members(l):
            if 0 <= int(m) <= 255:
                sel[cls[int(m)]] = True
        tp = int(hist[np.ix_(sel, sel)].sum())
        fp = int(hist[sel].sum()) - tp
        fn = int(hist[:, sel].sum()) - tp
        counts[str(l)] = (tp, fp, fn, total - tp - fp - fn)
    return counts


def _percentile_linear(lo_value, hi_value, gamma):
    """numpy's linear interpolation between two neighbouring order statistics (numpy.percentile, method 'linear')."""
    d = hi_value - lo_value
    return hi_value - d * (1 - gamma) if gamma >= 0.5 else lo_value + d * gamma


def _surface_metrics(t, r, members, counts, names, voxel_spacing, connectivity, nsd_tolerance=None):
    """The advanced metrics of one label entry (metrics.py:314-383 over medpy's hd / hd95 / asd / assd; NSD_METRIC at
    nsd_tolerance: surface_dice.py:43-56 on the same distances, one more launch and 16 bytes read back)."""
    tp, fp, fn, tn = counts
    nan = float("NaN")
    if (tp + fp) == 0 or (tn + fn) == 0 or (tp + fn) == 0 or (tn + fp) == 0:       # test / reference empty or full
        return OrderedDict((k, nan) for k in names)
    from .. import ops
    import torch
    member = np.zeros(256, dtype=bool)
    for m in members:
        if 0 <= int(m) <= 255:
            member[int(m)] = True
    capacity = 2 * tp + fp + fn                                 # border voxels are mask voxels
    with torch.cuda.device(t.device):
        sds, stats = ops.surface_distances(t, r, member, voxel_spacing, connectivity, capacity=capacity)
        n_tr, max_tr, sum_tr, n_rt, max_rt, sum_rt = (float(i) for i in stats.cpu())
        n_tr, n_rt = int(n_tr), int(n_rt)
        n = n_tr + n_rt
        assert 0 < n_tr and 0 < n_rt and n <= capacity, (n_tr, n_rt, capacity)
        res = OrderedDict()
        for k in names:
            if k == "Hausdorff Distance":
                res[k] = max(max_tr, max_rt)
            elif k == "Hausdorff Distance 95":
                pos = (n - 1) * 0.95                            # numpy.percentile(hstack((sds_tr, sds_rt)), 95)
                lo = min(int(np.floor(pos)), n - 1)
                hi = min(lo + 1, n - 1)
                v_lo, v_hi = (float(i) for i in ops.select_kth(sds[:n], [lo, hi]).cpu())
                res[k] = float(_percentile_linear(v_lo, v_hi, pos - lo))
            elif k == "Avg. Surface Distance":
                res[k] = sum_tr / n_tr
            elif k == "Avg. Symmetric Surface Distance":
                res[k] = float(np.mean((sum_tr / n_tr, sum_rt / n_rt)))
            elif k == NSD_METRIC:
                (c_tr,), (c_rt,) = ops.sd_count_within(sds, n_tr, n_rt, [nsd_tolerance]).cpu().tolist()
                res[k] = nsd_from_counts(c_tr, n_tr, c_rt, n_rt)
    return res


def _load(x):
    """-> (volume: numpy array or device tensor, file name or None, spacing (x, y, z) of a file or None).  With a HIP device a
    `.nii.gz` file is read through `read_image_device`: ground-truth label maps are inflated where they are compared."""
    if isinstance(x, str):
        import torch
        if torch.cuda.is_available() and x.endswith('.nii.gz'):
            vox, spacing, _, _ = read_image_device(x, torch.device('cuda', torch.cuda.current_device()))
            return vox, x, spacing
        img = read_image(x)
        return np.asarray(img.array), x, img.spacing
    if _is_device_tensor(x):
        return x, None, None
    try:
        import torch
        if torch.is_tensor(x):
            return x.numpy(), None, None
    except ImportError:
        pass
    return np.asarray(x), None, None


def evaluate_case(test_file, ref_file, labels, advanced=False, advanced_metrics=None, voxel_spacing=None, connectivity=1,
                  nsd_threshold=None):
    """labels: iterable of ints or tuples of ints (a tuple = the union of its members, evaluator.py:140-160).  test_file /
    ref_file: file names, numpy arrays or HIP device tensors.  advanced=True appends `advanced_metrics` (default
    DEFAULT_ADVANCED_METRICS; any of ADVANCED_METRICS) with `voxel_spacing` (z, y, x) - default: the test file's spacing, unit
    spacing for arrays (NiftiEvaluator.evaluate, evaluator.py:297-303) - and `connectivity` 1..3 of the erosion structure.
    `advanced_metrics` may also name NSD_METRIC; then `nsd_threshold` is its tolerance in mm: one number, or a dict
    {str(label): number} with an entry for every label."""
    labels = list(labels)
    nsd = {}
    if advanced and advanced_metrics is not None and NSD_METRIC in advanced_metrics:
        nsd = _nsd_tolerances(labels, nsd_threshold)            # before a file is read or the device is asked
    test, test_name, test_spacing = _load(test_file)
    ref, ref_name, _ = _load(ref_file)
    if tuple(test.shape) != tuple(ref.shape):
        raise ValueError("Shape mismatch: %s and %s" % (tuple(test.shape), tuple(ref.shape)))
    names = []
    if advanced:
        names = list(DEFAULT_ADVANCED_METRICS if advanced_metrics is None else advanced_metrics)
        for k in names:
            if k not in ADVANCED_METRICS and k != NSD_METRIC:
                raise ValueError("unknown advanced metric %r (one of %s)" % (k, ADVANCED_METRICS))
        if connectivity not in (1, 2, 3):
            raise ValueError("connectivity %r (1, 2 or 3)" % (connectivity,))
        if len(tuple(test.shape)) != 3:
            raise ValueError("advanced metrics need 3-D volumes [z, y, x], got shape %s" % (tuple(test.shape),))
        if voxel_spacing is None and test_spacing is not None:
            voxel_spacing = np.array(test_spacing, dtype=np.float64)[::-1]
        if voxel_spacing is not None:
            voxel_spacing = np.asarray(voxel_spacing, dtype=np.float64) * np.ones(3)
        import torch
        if not (torch.cuda.is_available() or _is_device_tensor(test) or _is_device_tensor(ref)):
            _no_device()
    pair = _device_pair(test, ref)
    res = OrderedDict()
    if pair is not None:
        counts = _device_counts(pair[0], pair[1], labels)
        for l in labels:
            res[str(l)] = metrics_from_counts(*counts[str(l)])
            if names:
                res[str(l)].update(_surface_metrics(pair[0], pair[1], _members(l), counts[str(l)], names, voxel_spacing,
                                                    connectivity, nsd.get(str(l))))
    else:
        if names:
            raise ValueError("advanced metrics need integer label volumes with values in 0..255")
        if _is_device_tensor(test):
            test = test.cpu().numpy()
        if _is_device_tensor(ref):
            ref = ref.cpu().numpy()
        for l in labels:
            members = l if isinstance(l, (tuple, list)) else (l,)
            t = np.isin(test, list(members))
            r = np.isin(ref, list(members))
            res[str(l)] = confusion_metrics(t, r)
    res["reference"] = ref_name
    res["test"] = test_name
    return res


def aggregate_scores(test_ref_pairs, labels=None, nanmean=True, json_output_file=None, json_name="", json_description="",
                     json_author="Fabian", json_task="", num_threads=2, evaluator=None, advanced=False, advanced_metrics=None,
                     voxel_spacing=None, connectivity=1, nsd_threshold=None):
    """evaluator.py:321-400.  `evaluator` and `num_threads` are accepted for the reference's callers and not used: the cases
    run one after another on the device.  Any other unknown keyword is a TypeError."""
    if labels is None:
        raise ValueError("labels must be given")
    scores = OrderedDict(all=[], mean=OrderedDict())
    for test, ref in test_ref_pairs:
        scores["all"].append(evaluate_case(test, ref, labels, advanced=advanced, advanced_metrics=advanced_metrics,
                                           voxel_spacing=voxel_spacing, connectivity=connectivity, nsd_threshold=nsd_threshold))
    for res in scores["all"]:
        for label, sd in res.items():
            if label in ("test", "reference"):
                continue
            dst = scores["mean"].setdefault(label, OrderedDict())
            for k, v in sd.items():
                dst.setdefault(k, []).append(v)
    for label in scores["mean"]:
        for k in scores["mean"][label]:
            v = scores["mean"][label][k]
            with np.errstate(all='ignore'):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    scores["mean"][label][k] = float(np.nanmean(v) if nanmean else np.mean(v))
    if json_output_file is not None:
        d = OrderedDict()
        d["name"], d["description"], d["timestamp"] = json_name, json_description, str(datetime.today())
        d["task"], d["author"], d["results"] = json_task, json_author, scores
        d["id"] = hashlib.md5(json.dumps(d).encode("utf-8")).hexdigest()[:12]
        with open(json_output_file, 'w') as f:
            json.dump(d, f, sort_keys=True, indent=4)
    return scores


def evaluate_folder(folder_with_gts, folder_with_predictions, labels, **metric_kwargs):
    """evaluator.py:446-461: every .nii.gz of the two folders (the names must match) -> summary.json in folder_with_predictions."""
    import os

    def subfiles(folder):
        return sorted(i for i in os.listdir(folder) if os.path.isfile(os.path.join(folder, i)) and i.endswith(".nii.gz"))
    files_gt, files_pred = subfiles(folder_with_gts), subfiles(folder_with_predictions)
    assert all(i in files_pred for i in files_gt), "files missing in folder_with_predictions"
    assert all(i in files_gt for i in files_pred), "files missing in folder_with_gts"
    test_ref_pairs = [(os.path.join(folder_with_predictions, i), os.path.join(folder_with_gts, i)) for i in files_pred]
    return aggregate_scores(test_ref_pairs, json_output_file=os.path.join(folder_with_predictions, "summary.json"), num_threads=8,
                            labels=labels, **metric_kwargs)


def main(argv=None):
    """The reference's nnunet_evaluate_folder (evaluator.py:464-483), plus --advanced and --nsd."""
    import argparse
    parser = argparse.ArgumentParser("Evaluates the segmentations located in the folder pred. Output of this script is a json "
                                     "file. At the very bottom of the json file is going to be a 'mean' entry with averages "
                                     "metrics across all cases")
    parser.add_argument('-ref', required=True, type=str, help="Folder containing the reference segmentations in nifti format.")
    parser.add_argument('-pred', required=True, type=str, help="Folder containing the predicted segmentations in nifti format. "
                                                               "File names must match between the folders!")
    parser.add_argument('-l', nargs='+', type=int, required=True, help="List of label IDs (integer values) that should be evaluated.")
    parser.add_argument('--advanced', action='store_true', help="Also the surface-distance metrics (HIP device only).")
    parser.add_argument('--advanced_metrics', nargs='+', default=None, help="Any of: %s" % ", ".join(repr(i) for i in ADVANCED_METRICS))
    parser.add_argument('--connectivity', type=int, default=1)
    parser.add_argument('--nsd', type=float, default=None, metavar='TOL', help="Also %r at this tolerance in mm (HIP device only)."
                                                                               % NSD_METRIC)
    args = parser.parse_args(argv)
    kw = dict(advanced=True, advanced_metrics=args.advanced_metrics, connectivity=args.connectivity) if args.advanced else {}
    if args.nsd is not None:
        names = list(kw['advanced_metrics'] or DEFAULT_ADVANCED_METRICS) if kw else []
        kw = dict(advanced=True, advanced_metrics=names + [NSD_METRIC] * (NSD_METRIC not in names), connectivity=args.connectivity,
                  nsd_threshold=args.nsd)
    return evaluate_folder(args.ref, args.pred, args.l, **kw)


if __name__ == '__main__':
    main()
