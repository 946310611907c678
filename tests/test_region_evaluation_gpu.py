"""Region-based evaluation on the device: `evaluate_regions` on the seeded folders of tests/region_cases.py (four predicted
24 x 40 x 48 cases with labels 0..3: a region absent from both volumes, regions absent from the prediction only, a ground truth
without prediction) writes the `summary.csv` of the REAL reference (tests/golden/region_evaluation.json,
tools/oracle_gen/make_golden_region_evaluation.py), byte for byte: the Dice values are ratios of exact integer counts in medpy's
operation order, so there is nothing to bound.  One inflated upload and one joint-histogram launch per case for all regions;
`summary_nsd.csv` only on request, its cells the evaluator's normalized surface Dice under %02.4f."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import region_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu
NSD = "Normalized Surface Dice"
GOLD = json.load(open(os.path.join(HERE, 'golden', 'region_evaluation.json')))


@pytest.fixture(scope='module')
def folders(tmp_path_factory):
    base = tmp_path_factory.mktemp('regions')
    pred, gt = base / 'pred', base / 'gt'
    pred.mkdir()
    gt.mkdir()
    names = RC.write_folders(str(pred), str(gt))
    assert names == ['case_00', 'case_01', 'case_02', 'case_03'] and len(os.listdir(str(gt))) == 5
    return str(pred), str(gt)


def test_cases_hold_what_the_docstring_says():
    assert GOLD['shape'] == list(RC.SHAPE) == [24, 40, 48]
    for c in RC.CASES[:4]:
        pred, gt = RC.region_case(c['seed'], c['pred_labels'], c['gt_labels'])
        assert sorted(np.unique(pred).tolist()) == [0] + list(c['pred_labels'])
        assert sorted(np.unique(gt).tolist()) == [0] + list(c['gt_labels'])
    assert RC.region_case(25, None, (1, 2, 3))[0] is None


def test_summary_csv_is_the_references(dev, folders, monkeypatch, capsys):
    from multitalent_amd import ops
    from multitalent_amd.evaluation import evaluator as E
    from multitalent_amd.evaluation import region_based_evaluation as R
    pred, gt = folders
    calls = {'hist': 0, 'read': 0}
    real_hist, real_read = ops.seg_joint_hist, E.read_image_device
    monkeypatch.setattr(ops, 'seg_joint_hist', lambda *a, **k: calls.__setitem__('hist', calls['hist'] + 1) or real_hist(*a, **k))
    monkeypatch.setattr(E, 'read_image_device', lambda *a, **k: calls.__setitem__('read', calls['read'] + 1) or real_read(*a, **k))

    def boom(*a, **k):
        raise AssertionError("no surface launch without nsd_threshold")
    monkeypatch.setattr(ops, 'surface_distances', boom)
    for key, regions in (('kits', R.get_KiTS_regions()), ('brats', R.get_brats_regions())):
        assert {k: list(v) for k, v in regions.items()} == GOLD[key]['regions']
        calls.update(hist=0, read=0)
        R.evaluate_regions(pred, gt, regions, processes=4)
        assert calls == {'hist': 4, 'read': 8}                   # per case: both files inflated on the device, one histogram
        assert open(os.path.join(pred, 'summary.csv')).read() == GOLD[key]['summary_csv']
        assert "WARNING! Some files in folder_gt were not predicted" in capsys.readouterr().out
        assert not os.path.exists(os.path.join(pred, 'summary_nsd.csv'))
    # one case, by file name, array and device tensor: the same list
    import torch
    c = RC.CASES[2]
    p, g = RC.region_case(c['seed'], c['pred_labels'], c['gt_labels'])
    by_file = R.evaluate_case(os.path.join(pred, 'case_02.nii.gz'), os.path.join(gt, 'case_02.nii.gz'), [(1, 2), (2,)])
    assert by_file == R.evaluate_case(p, g, [(1, 2), (2,)]) == R.evaluate_case(torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev),
                                                                               [[1, 2], [2]])
    assert 0.0 < by_file[0] < 1.0 and by_file[1] == 0.0
    m = R.create_region_from_mask(torch.from_numpy(g).to(dev), (2, 3))
    assert m.is_cuda and m.dtype == torch.uint8 and np.array_equal(m.cpu().numpy(), np.isin(g, (2, 3)).astype(np.uint8))


def test_prediction_without_ground_truth(dev, folders, tmp_path):
    from multitalent_amd.evaluation import region_based_evaluation as R
    from multitalent_amd.utilities import nifti_io
    pred, gt = folders
    lonely = tmp_path / 'pred'
    lonely.mkdir()
    nifti_io.write_image(np.zeros(RC.SHAPE, np.uint8), str(lonely / 'case_99.nii.gz'))
    with pytest.raises(AssertionError, match="have not ground truth"):
        R.evaluate_regions(str(lonely), gt, R.get_KiTS_regions())
    assert not os.path.exists(str(lonely / 'summary.csv'))


def test_summary_nsd_csv_on_request(dev, folders, tmp_path):
    from multitalent_amd.evaluation import evaluator as E
    from multitalent_amd.evaluation import region_based_evaluation as R
    pred, gt = folders
    regions = R.get_KiTS_regions()
    tol = {'kidney incl tumor': 2.0, 'tumor': 3.5}
    R.evaluate_regions(pred, gt, regions, nsd_threshold=tol)
    try:
        text = open(os.path.join(pred, 'summary_nsd.csv')).read()
        assert open(os.path.join(pred, 'summary.csv')).read() == GOLD['kits']['summary_csv']
    finally:
        os.remove(os.path.join(pred, 'summary_nsd.csv'))
    lines = text.split("\n")
    assert lines[0] == "casename,kidney incl tumor,tumor" and lines[-1] == "" and len(lines) == 10
    assert [l.split(",")[0] for l in lines[5:9]] == ['mean', 'median', 'mean (nan is 1)', 'median (nan is 1)']
    cols = [[], []]
    for i, name in enumerate(['case_00', 'case_01', 'case_02', 'case_03']):
        labels = [tuple(r) for r in regions.values()]
        res = E.evaluate_case(os.path.join(pred, name + '.nii.gz'), os.path.join(gt, name + '.nii.gz'), labels, advanced=True,
                              advanced_metrics=[NSD], nsd_threshold={str(l): tol[n] for l, n in zip(labels, regions)})
        assert lines[1 + i] == name + "".join(",%02.4f" % res[str(l)][NSD] for l in labels)
        for k, l in enumerate(labels):
            cols[k].append(res[str(l)][NSD])
    assert lines[2].endswith(",nan") and lines[3].endswith(",nan")          # no tumor border: both empty / prediction empty
    assert lines[5] == "mean" + "".join(",%02.4f" % np.nanmean(c) for c in cols)
    assert lines[8] == "median (nan is 1)" + "".join(",%02.4f" % np.median(np.where(np.isnan(c), 1.0, c)) for c in cols)
    # the command line: kits by name, the same regions from a json file, and --nsd
    rj = str(tmp_path / 'regions.json')
    with open(rj, 'w') as f:
        json.dump({"kidney incl tumor": [1, 2], "tumor": [2]}, f)
    for which in ('kits', rj):
        os.remove(os.path.join(pred, 'summary.csv'))
        R.main(['-pred', pred, '-ref', gt, '--regions', which])
        assert open(os.path.join(pred, 'summary.csv')).read() == GOLD['kits']['summary_csv']
        assert not os.path.exists(os.path.join(pred, 'summary_nsd.csv'))
    R.main(['-pred', pred, '-ref', gt, '--regions', 'brats', '--nsd', '2.0'])
    try:
        assert open(os.path.join(pred, 'summary.csv')).read() == GOLD['brats']['summary_csv']
        head = open(os.path.join(pred, 'summary_nsd.csv')).read().split("\n")[0]
        assert head == "casename,whole tumor,tumor core,enhancing tumor"
    finally:
        os.remove(os.path.join(pred, 'summary_nsd.csv'))
