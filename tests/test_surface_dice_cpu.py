"""Normalized surface Dice and region-based evaluation, host side (no GPU): the formula on integer counts against a float64
numpy restatement of the reference's surface_dice.py:46-55 (==), the argument errors, the region tables, the csv writer against
text written by hand, `evaluate_regions` through the evaluator's host loop against the golden of the real reference
(tests/golden/region_evaluation.json, tools/oracle_gen/make_golden_region_evaluation.py), and the new C entry's declaration."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evaluation_cases as EC  # noqa: E402
import region_cases as RC  # noqa: E402

NSD = "Normalized Surface Dice"


def _numpy_nsd(a_to_b, b_to_a, threshold):
    """surface_dice.py:46-55 on two float64 arrays of distances"""
    numel_a, numel_b = len(a_to_b), len(b_to_a)
    tp_a = np.sum(a_to_b <= threshold) / numel_a
    tp_b = np.sum(b_to_a <= threshold) / numel_b
    fp = np.sum(a_to_b > threshold) / numel_a
    fn = np.sum(b_to_a > threshold) / numel_b
    return (tp_a + tp_b) / (tp_a + tp_b + fp + fn + 1e-8)


def test_formula_on_counts_equals_numpy():
    from multitalent_amd.evaluation.evaluator import nsd_from_counts
    rng = np.random.default_rng(0)
    for n_a, n_b in ((1, 1), (1, 7), (3, 2), (97, 1001), (12345, 54321), (3, 10 ** 6)):
        for thr in (0.0, 0.3, 1.0, 2.5, np.inf):
            a = np.round(rng.random(n_a) * 4, 1)                # multiples of 0.1: many values equal to 0.3, 1.0, 2.5 and 0
            b = np.round(rng.random(n_b) * 4, 1)
            got = nsd_from_counts(int((a <= thr).sum()), n_a, int((b <= thr).sum()), n_b)
            want = _numpy_nsd(a, b, thr)
            assert isinstance(got, float) and got == float(want), (n_a, n_b, thr, got, want)
    assert nsd_from_counts(0, 5, 0, 9) == 0.0
    assert nsd_from_counts(5, 5, 9, 9) == 2.0 / (2.0 + 1e-8)
    assert abs(nsd_from_counts(7, 9, 2, 3) - nsd_from_counts(2, 3, 7, 9)) <= 1e-15         # symmetric up to one rounding of the sum


def test_argument_errors_come_before_the_device(monkeypatch):
    import torch
    from multitalent_amd.evaluation import evaluator as E
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    t, r = EC.golden_case(11)
    assert E.NSD_METRIC == NSD and NSD not in E.ADVANCED_METRICS and len(E.ADVANCED_METRICS) == 4
    with pytest.raises(ValueError, match="nsd_threshold"):                          # no tolerance at all
        E.evaluate_case(t, r, [1], advanced=True, advanced_metrics=[NSD])
    with pytest.raises(ValueError, match="nsd_threshold"):                          # none for the tuple entry
        E.evaluate_case(t, r, [1, (1, 2)], advanced=True, advanced_metrics=[NSD], nsd_threshold={'1': 2.0})
    for bad in (float('nan'), -1.0, 'two', {'1': float('nan')}):
        with pytest.raises(ValueError, match="nsd_threshold"):
            E.evaluate_case(t, r, [1], advanced=True, advanced_metrics=[NSD], nsd_threshold=bad)
    with pytest.raises(ValueError, match="nsd_threshold"):
        E.aggregate_scores([(t, r)], labels=[1, 2], advanced=True, advanced_metrics=["Hausdorff Distance", NSD])
    with pytest.raises(ValueError, match="nsd_threshold"):                          # not even the file is opened
        E.evaluate_case('/nonexistent/a.nii.gz', '/nonexistent/b.nii.gz', [1], advanced=True, advanced_metrics=[NSD])
    with pytest.raises(ValueError, match="unknown advanced metric"):
        E.evaluate_case(t, r, [1], advanced=True, advanced_metrics=["Hausdorf", NSD], nsd_threshold=1.0)
    with pytest.raises(ValueError, match="unknown advanced metric"):
        E.evaluate_case(t, r, [1], advanced=True, advanced_metrics=["normalized surface dice"], nsd_threshold=1.0)
    # complete arguments: the existing refusal of a machine without a HIP device
    with pytest.raises(RuntimeError, match="HIP device only"):
        E.evaluate_case(t, r, [1, (1, 2)], advanced=True, advanced_metrics=[NSD], nsd_threshold={'1': 2.0, '(1, 2)': 0.0})
    from multitalent_amd.evaluation.surface_dice import normalized_surface_dice
    with pytest.raises(RuntimeError, match="HIP device only"):
        normalized_surface_dice(t > 0, r > 0, 2.0, (1, 1, 1))
    with pytest.raises(AssertionError):
        normalized_surface_dice(t[1:], r, 2.0)
    # a tolerance is ignored, not an error, when the metric is not asked for
    assert len(E.evaluate_case(t, r, [1], nsd_threshold=3.0)['1']) == 13


def test_count_op_refuses_bad_arguments_without_a_device():
    import torch
    from multitalent_amd import ops
    x = torch.zeros(8, dtype=torch.float64)
    for n_tr, n_rt, tols in ((4, 4, []), (4, 4, [1.0] * 9), (4, 4, [float('nan')]), (4, 4, [1.0, -0.5]), (0, 0, [1.0]), (-1, 4, [1.0]),
                             (4, -1, [1.0]), (5, 4, [1.0])):
        with pytest.raises(ValueError, match="sd_count_within"):
            ops.sd_count_within(x, n_tr, n_rt, tols)
    with pytest.raises(RuntimeError, match="HIP device only"):                      # valid arguments, host tensor
        ops.sd_count_within(x, 4, 4, [1.0, float('inf')])


def test_entry_is_declared_and_bound():
    import ctypes as C
    from multitalent_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(HERE, '..', 'include', 'mtseg.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+mt_sd_count_within\s*\(([^;]*?)\)\s*;', txt)
    assert m and 'mt_sd_count_within' in _lib.SIGNATURES
    res, args = _lib.SIGNATURES['mt_sd_count_within']
    assert res is C.c_int and len(args) == len(m.group(1).split(',')) == 7
    lib = _lib.load()
    assert hasattr(lib, 'mt_sd_count_within') and lib.mt_abi_version() == _lib.MT_ABI_VERSION == 4
    # the refusals of the entry itself need no device: nothing is launched, nothing is dereferenced on the device
    buf = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    cnt = (C.c_int64 * 16)()
    one, nan, neg, nine = (C.c_double * 1)(1.0), (C.c_double * 1)(float('nan')), (C.c_double * 1)(-1.0), (C.c_double * 9)(*([1.0] * 9))
    p = lambda a: C.cast(a, C.c_void_p)                          # noqa: E731
    for sds, n_tr, n_rt, tols, T, out in ((None, 2, 2, one, 1, cnt), (buf, 2, 2, None, 1, cnt), (buf, 2, 2, one, 1, None),
                                          (buf, 2, 2, one, 0, cnt), (buf, 2, 2, nine, 9, cnt), (buf, 0, 0, one, 1, cnt),
                                          (buf, -1, 2, one, 1, cnt), (buf, 2, -1, one, 1, cnt), (buf, 2, 2, nan, 1, cnt),
                                          (buf, 2, 2, neg, 1, cnt)):
        rc = lib.mt_sd_count_within(p(sds) if sds is not None else None, n_tr, n_rt, p(tols) if tols is not None else None, T,
                                    p(out) if out is not None else None, None)
        assert rc == -1 and b"sd_count_within" in lib.mt_last_error(), (n_tr, n_rt, T)             # MT_EINVAL


def test_region_tables():
    from multitalent_amd.evaluation import region_based_evaluation as R
    assert R.get_KiTS_regions() == {"kidney incl tumor": (1, 2), "tumor": (2,)}
    assert list(R.get_KiTS_regions()) == ["kidney incl tumor", "tumor"]
    assert R.get_brats_regions() == {"whole tumor": (1, 2, 3), "tumor core": (2, 3), "enhancing tumor": (3,)}
    assert list(R.get_brats_regions()) == ["whole tumor", "tumor core", "enhancing tumor"]
    m = np.array([[0, 1, 2], [3, 2, 5]], dtype=np.int16)
    out = R.create_region_from_mask(m, (2, 3))
    assert out.dtype == np.uint8 and out.tolist() == [[0, 0, 1], [1, 1, 0]]
    # Dice per region: NaN for two empty masks, 0.0 when one is empty, medpy's 2 |A & B| / (|A| + |B|) otherwise
    assert math.isnan(R.dice_from_counts(0, 0, 0))
    assert R.dice_from_counts(0, 0, 17) == 0.0 and R.dice_from_counts(0, 17, 0) == 0.0
    assert R.dice_from_counts(3, 2, 4) == 2. * 3 / float(5 + 7)


CSV_WANT = ("casename,kidney incl tumor,tumor,never\n"
            "a,0.5000,nan,nan\n"
            "b,1.0000,0.1235,nan\n"
            "c,0.0000,0.6667,nan\n"
            "mean,0.5000,0.3951,nan\n"
            "median,0.5000,0.3951,nan\n"
            "mean (nan is 1),0.5000,0.5967,1.0000\n"
            "median (nan is 1),0.5000,0.6667,1.0000\n")


def test_csv_writer_against_text_written_by_hand(tmp_path):
    """Column 2 has one NaN, column 3 nothing else: mean / median skip NaN (nan for the empty column), the 'nan is 1' rows count it
    as 1.  0.12345 rounds to 0.1235 under %02.4f (the double lies above the tie), 2/3 to 0.6667."""
    from multitalent_amd.evaluation.region_based_evaluation import write_summary_csv
    nan = float('nan')
    f = str(tmp_path / 'summary.csv')
    write_summary_csv(f, ['a', 'b', 'c'], ['kidney incl tumor', 'tumor', 'never'],
                      [[0.5, nan, nan], [1.0, 0.12345, nan], [0.0, 2 / 3, nan]])
    assert open(f).read() == CSV_WANT


def test_evaluate_regions_host_loop_equals_the_reference(tmp_path, monkeypatch, capsys):
    """No device: the evaluator's host loop counts; the csv is the real reference's, byte for byte."""
    import torch
    from multitalent_amd.evaluation import region_based_evaluation as R
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    gold = json.load(open(os.path.join(HERE, 'golden', 'region_evaluation.json')))
    assert gold['shape'] == list(RC.SHAPE) and [c['name'] for c in gold['cases']] == [c['name'] for c in RC.CASES]
    pred, gt = tmp_path / 'pred', tmp_path / 'gt'
    pred.mkdir()
    gt.mkdir()
    RC.write_folders(str(pred), str(gt))
    for key, regions in (('kits', R.get_KiTS_regions()), ('brats', R.get_brats_regions())):
        assert {k: list(v) for k, v in regions.items()} == gold[key]['regions']
        R.evaluate_regions(str(pred), str(gt), regions, processes=3)
        assert open(str(pred / 'summary.csv')).read() == gold[key]['summary_csv']
        assert "WARNING! Some files in folder_gt were not predicted" in capsys.readouterr().out
        assert not os.path.exists(str(pred / 'summary_nsd.csv'))
    with pytest.raises(RuntimeError, match="HIP device only"):
        R.evaluate_regions(str(pred), str(gt), R.get_KiTS_regions(), nsd_threshold=2.0)
    with pytest.raises(ValueError, match="nsd_threshold"):
        R.evaluate_regions(str(pred), str(gt), R.get_KiTS_regions(), nsd_threshold={'tumor': 2.0})
    os.remove(str(gt / 'case_02.nii.gz'))
    with pytest.raises(AssertionError, match="have not ground truth"):
        R.evaluate_regions(str(pred), str(gt), R.get_KiTS_regions())
