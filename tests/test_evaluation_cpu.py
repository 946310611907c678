"""Evaluation, host side (no GPU): counts -> metrics, the scipy restatement of medpy's surface distances against answers that
can be computed by hand, and the keyword handling of aggregate_scores."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluation_cases as EC  # noqa: E402


def _same(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert (math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], (k, a[k], b[k])


def test_metrics_from_counts_equals_confusion_metrics():
    from multitalent_amd.evaluation.evaluator import DEFAULT_METRICS, confusion_metrics, metrics_from_counts
    rng = np.random.default_rng(0)
    shape = (6, 7, 8)
    pairs = [(rng.random(shape) < p, rng.random(shape) < q) for p, q in ((0.3, 0.4), (0.05, 0.9), (0.5, 0.5), (0.99, 0.01))]
    zeros, ones = np.zeros(shape, bool), np.ones(shape, bool)
    some = rng.random(shape) < 0.3
    pairs += [(zeros, some), (some, zeros), (ones, some), (some, ones), (zeros, zeros), (ones, ones), (zeros, ones)]
    for t, r in pairs:
        tp, fp, fn = int((t & r).sum()), int((t & ~r).sum()), int((~t & r).sum())
        m = metrics_from_counts(tp, fp, fn, t.size - tp - fp - fn)
        assert list(m.keys()) == DEFAULT_METRICS
        _same(m, confusion_metrics(t, r))
    # the four NaN situations by name
    n = some.size
    k = int(some.sum())
    assert math.isnan(metrics_from_counts(0, 0, k, n - k)["Precision"])                      # test empty
    assert math.isnan(metrics_from_counts(0, k, 0, n - k)["Recall"])                         # reference empty
    assert math.isnan(metrics_from_counts(k, n - k, 0, 0)["False Omission Rate"])            # test full
    assert math.isnan(metrics_from_counts(k, 0, n - k, 0)["True Negative Rate"])             # reference full
    assert math.isnan(metrics_from_counts(0, 0, 0, n)["Dice"])                               # both empty


def test_scipy_restatement_two_single_voxels():
    a, b = np.zeros((9, 10, 11), bool), np.zeros((9, 10, 11), bool)
    a[1, 2, 3] = True
    b[7, 4, 9] = True
    sp = (3.0, 1.0, 0.7)
    want = math.sqrt((6 * 3.0) ** 2 + (2 * 1.0) ** 2 + (6 * 0.7) ** 2)
    for conn in (1, 2, 3):
        for f in (EC.hd, EC.hd95, EC.asd, EC.assd):
            assert f(a, b, sp, conn) == pytest.approx(want, rel=1e-14)
    assert EC.hd(a, b, None, 1) == pytest.approx(math.sqrt(36 + 4 + 36), rel=1e-14)


def test_scipy_restatement_two_boxes():
    """Boxes [2, 6) x [3, 9) x [4, 12) and [10, 14) x [3, 9) x [4, 12): the faces that look at each other are 4 voxels apart, the
    far faces 8; every border voxel of one box has its nearest border voxel of the other straight across in z."""
    a, b = np.zeros((16, 12, 16), bool), np.zeros((16, 12, 16), bool)
    a[2:6, 3:9, 4:12] = True
    b[10:14, 3:9, 4:12] = True
    sp = (2.0, 1.0, 1.0)
    assert EC.hd(a, b, sp, 1) == 2.0 * 8                    # from a's far face z = 2 to b's near face z = 10
    assert EC.hd(a, b, None, 1) == 8.0
    s = EC.surface_distances_scipy(a, b, None, 1)
    assert s.min() == 5.0 and s.max() == 8.0                # a's near face z = 5 to z = 10
    assert len(s) == 4 * 6 * 8 - 2 * 4 * 6                  # all but the interior
    assert EC.assd(a, b, None, 1) == pytest.approx(EC.asd(a, b, None, 1))    # the mirror image


def test_advanced_without_a_device_raises(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    from multitalent_amd.evaluation.evaluator import aggregate_scores, evaluate_case
    t, r = EC.golden_case(11)
    with pytest.raises(RuntimeError, match="HIP device only"):
        aggregate_scores([(t, r)], labels=[1, 2], advanced=True)
    with pytest.raises(RuntimeError, match="HIP device only"):
        evaluate_case(t, r, [1], advanced=True, advanced_metrics=["Hausdorff Distance"])


def test_aggregate_scores_keywords():
    from multitalent_amd.evaluation.evaluator import aggregate_scores
    t, r = EC.golden_case(11)
    base = aggregate_scores([(t, r)], labels=[1, (1, 2)])
    _same(base['mean']['1'], aggregate_scores([(t, r)], labels=[1, (1, 2)], evaluator=None, num_threads=8)['mean']['1'])
    with pytest.raises(TypeError):
        aggregate_scores([(t, r)], labels=[1], advance=True)
    with pytest.raises(ValueError):
        aggregate_scores([(t, r)], labels=[1], advanced=True, advanced_metrics=["Hausdorf"])
