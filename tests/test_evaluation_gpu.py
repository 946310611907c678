"""Evaluation on the device: the joint label histogram against numpy (exact), evaluate_case's device counts against the host
path (==), the surface distances against the scipy restatement of medpy's algorithm (tests/evaluation_cases.py), the NaN rules,
the goldens of the real reference's evaluator (tests/golden/evaluation.json, tools/oracle_gen/make_golden_evaluation.py) and
evaluate_folder.

Bounds: counts and the thirteen default metrics are integers through one shared formula: exact.  Every surface distance, hd and
hd95: relative 1e-12 against scipy (both sides evaluate the same fp64 expression at a nearest site; equidistant sites differ by a
few ulp; an fp32 step anywhere would be 1e-7).  asd, assd: relative 1e-10 (a sum of n <= 1.5e5 non-negative fp64 terms in any
fixed order is within (n - 1) 2^-53 <= 1.7e-11 of exact).  Run to run: bit-identical.
The surface-distance numbers are UNPINNED against medpy itself (third party, not vendored by the reference): the oracle is the
restatement of its published algorithm with scipy."""
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluation_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluation.json')


def _np_hist(t, r, remap, C):
    remap = np.asarray(remap, dtype=np.int64)
    idx = remap[t.ravel().astype(np.int64)] * C + remap[r.ravel().astype(np.int64)]
    return np.bincount(idx, minlength=C * C).reshape(C, C)


def _hist_dev(t, r, remap, C, dev):
    import torch
    from multitalent_amd import ops
    td, rd = torch.from_numpy(t).to(dev), torch.from_numpy(r).to(dev)
    h1 = ops.seg_joint_hist(td, rd, remap, C).cpu().numpy()
    h2 = ops.seg_joint_hist(td, rd, remap, C).cpu().numpy()
    assert np.array_equal(h1, h2)
    return h1


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 5, 7), (37, 61, 83), (64, 128, 128)])
def test_joint_hist_random(dev, shape):
    rng = np.random.default_rng(sum(shape))
    t = rng.integers(0, 6, shape).astype(np.uint8)
    r = rng.integers(0, 6, shape).astype(np.uint8)
    ident = np.minimum(np.arange(256), 5)
    merge = np.array([0, 1, 1, 2, 0, 2] + [0] * 250)
    for remap, C in ((ident, 6), (merge, 3), (np.arange(256), 256)):
        h = _hist_dev(t, r, remap, C, dev)
        assert h.dtype == np.int64 and int(h.sum()) == t.size
        assert np.array_equal(h, _np_hist(t, r, remap, C))


def test_joint_hist_400_cubed_mostly_background(dev):
    rng = np.random.default_rng(5)
    n = 400
    t = (rng.integers(1, 5, (n, n, n)) * (rng.random((n, n, n)) < 0.05)).astype(np.uint8)
    r = t.copy()
    flip = rng.random((n, n, n)) < 0.01
    r[flip] = rng.integers(0, 5, int(flip.sum())).astype(np.uint8)
    remap = np.minimum(np.arange(256), 4)
    assert np.array_equal(_hist_dev(t, r, remap, 5, dev), _np_hist(t, r, remap, 5))


def test_joint_hist_constant_volumes_and_wide_tables(dev):
    rng = np.random.default_rng(6)
    shape = (20, 33, 47)
    zeros = np.zeros(shape, np.uint8)
    threes = np.full(shape, 3, np.uint8)
    ident8 = np.minimum(np.arange(256), 7)
    for t, r in ((zeros, zeros), (threes, threes), (zeros, threes)):
        for remap, C in ((ident8, 8), (np.arange(256), 256), (np.arange(256) % 65, 65)):
            assert np.array_equal(_hist_dev(t, r, remap, C, dev), _np_hist(t, r, remap, C))
    t = rng.integers(0, 256, shape).astype(np.uint8)                     # values up to 255: C > 64, the global-atomic path
    r = rng.integers(0, 256, shape).astype(np.uint8)
    for remap, C in ((np.arange(256), 256), (np.arange(256) % 100, 100), (np.arange(256) % 64, 64)):
        assert np.array_equal(_hist_dev(t, r, remap, C, dev), _np_hist(t, r, remap, C))


def test_joint_hist_unaligned_slices(dev):
    import torch
    from multitalent_amd import ops
    rng = np.random.default_rng(8)
    n = 100003
    a = rng.integers(0, 4, n + 64).astype(np.uint8) * (rng.random(n + 64) < 0.3)
    b = rng.integers(0, 4, n + 64).astype(np.uint8) * (rng.random(n + 64) < 0.3)
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    remap = np.minimum(np.arange(256), 3)
    for oa, ob, length in ((1, 1, n), (3, 3, n - 5), (5, 9, n), (0, 7, 1001), (13, 13, 9), (2, 2, 31)):
        ta, tb = ad[oa:oa + length], bd[ob:ob + length]
        assert ta.is_contiguous() and ta.data_ptr() % 16 == oa % 16
        h = ops.seg_joint_hist(ta, tb, remap, 4).cpu().numpy()
        assert np.array_equal(h, _np_hist(a[oa:oa + length], b[ob:ob + length], remap, 4)), (oa, ob, length)


def _same_metrics(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert (math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], (k, a[k], b[k])


def _host_case(monkeypatch, *args, **kw):
    """evaluate_case through the host loop: the device is hidden from the evaluator for this call"""
    import torch
    from multitalent_amd.evaluation.evaluator import evaluate_case
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, 'is_available', lambda: False)
        return evaluate_case(*args, **kw)


def test_evaluate_case_device_counts_equal_host(dev, monkeypatch, tmp_path):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.evaluation import evaluator as E
    from multitalent_amd.utilities import nifti_io
    rng = np.random.default_rng(3)
    shape = (19, 40, 33)
    test = (rng.integers(0, 5, shape) * (rng.random(shape) < 0.4)).astype(np.int16)
    ref = (rng.integers(0, 5, shape) * (rng.random(shape) < 0.4)).astype(np.uint8)
    labels = [0, 1, 2, 3, 4, 7, (1, 2), (3, 4, 9), (0, 1), 300]
    host = _host_case(monkeypatch, test, ref, labels)
    calls = []
    real = ops.seg_joint_hist
    monkeypatch.setattr(ops, 'seg_joint_hist', lambda *a, **k: calls.append(1) or real(*a, **k))
    devr = E.evaluate_case(test, ref, labels)
    assert len(calls) == 1                                           # all labels: one launch
    tens = E.evaluate_case(torch.from_numpy(test).to(dev), torch.from_numpy(ref).to(dev), labels)
    assert len(calls) == 2
    assert list(host.keys()) == list(devr.keys()) == list(tens.keys())
    for l in labels:
        _same_metrics(host[str(l)], devr[str(l)])
        _same_metrics(host[str(l)], tens[str(l)])
    tf, rf = str(tmp_path / 'test.nii.gz'), str(tmp_path / 'ref.nii.gz')
    nifti_io.write_image(test.astype(np.uint8), tf, (0.7, 0.8, 2.5))
    nifti_io.write_image(ref, rf, (0.7, 0.8, 2.5))
    hostf = _host_case(monkeypatch, tf, rf, labels)
    devf = E.evaluate_case(tf, rf, labels)
    assert len(calls) == 3 and devf['test'] == tf and devf['reference'] == rf
    for l in labels:
        _same_metrics(hostf[str(l)], devf[str(l)])
        _same_metrics(host[str(l)], devf[str(l)])
    # values outside 0..255: the host loop, as before
    big = test.astype(np.int32) + 1000 * (test == 4)
    _same_metrics(E.evaluate_case(big, ref, [1, 1004])['1004'], _host_case(monkeypatch, big, ref, [1, 1004])['1004'])
    assert len(calls) == 3


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.abs(a - b) / np.abs(b)
    return float(np.max(np.where(a == b, 0.0, r))) if a.size else 0.0


def _check_surface(a, b, spacing, conn, dev):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.evaluation.evaluator import evaluate_case
    t = torch.from_numpy(a.astype(np.uint8) * 5).to(dev)
    r = torch.from_numpy(b.astype(np.uint8) * 5).to(dev)
    member = np.zeros(256, bool)
    member[5] = True
    s_tr = EC.surface_distances_scipy(a, b, spacing, conn)
    s_rt = EC.surface_distances_scipy(b, a, spacing, conn)
    cap = int(a.sum()) + int(b.sum())
    out, stats = ops.surface_distances(t, r, member, spacing, conn, capacity=cap)
    out2, stats2 = ops.surface_distances(t, r, member, spacing, conn)               # default capacity, second run
    st = stats.cpu().numpy()
    n_tr, n_rt = int(st[0]), int(st[3])
    print("border voxels %d + %d" % (n_tr, n_rt))
    assert (n_tr, n_rt) == (len(s_tr), len(s_rt))
    d = out[:n_tr + n_rt].cpu().numpy()
    assert np.array_equal(d, out2[:n_tr + n_rt].cpu().numpy()) and np.array_equal(st, stats2.cpu().numpy())    # bit-identical
    figures = {'sorted t->r': _rel(np.sort(d[:n_tr]), np.sort(s_tr)), 'sorted r->t': _rel(np.sort(d[n_tr:]), np.sort(s_rt)),
               'in order': _rel(d, np.hstack((s_tr, s_rt))),
               'max': max(_rel(st[1], s_tr.max()), _rel(st[4], s_rt.max())),
               'sum': max(_rel(st[2], s_tr.sum()), _rel(st[5], s_rt.sum()))}
    res = evaluate_case(t, r, [5], advanced=True, advanced_metrics=EC.ADVANCED, voxel_spacing=spacing, connectivity=conn)['5']
    want = {'Hausdorff Distance': EC.hd(a, b, spacing, conn), 'Hausdorff Distance 95': EC.hd95(a, b, spacing, conn),
            'Avg. Surface Distance': EC.asd(a, b, spacing, conn), 'Avg. Symmetric Surface Distance': EC.assd(a, b, spacing, conn)}
    for k in EC.ADVANCED:
        figures[k] = _rel(res[k], want[k])
    print(figures)
    # order statistics straight from the radix select against the sorted scipy array
    allsorted = np.sort(np.hstack((s_tr, s_rt)))
    n = len(allsorted)
    ranks = sorted({0, n - 1, n // 2, int(0.95 * (n - 1)), min(n - 1, int(0.95 * (n - 1)) + 1)})
    kth = ops.select_kth(out[:n], ranks).cpu().numpy()
    assert np.array_equal(kth, np.sort(d)[ranks])
    assert _rel(kth, allsorted[ranks]) <= 1e-12
    assert figures['sorted t->r'] <= 1e-12 and figures['sorted r->t'] <= 1e-12 and figures['in order'] <= 1e-12
    assert figures['max'] <= 1e-12 and figures['sum'] <= 1e-10
    assert figures['Hausdorff Distance'] <= 1e-12 and figures['Hausdorff Distance 95'] <= 1e-12
    assert figures['Avg. Surface Distance'] <= 1e-10 and figures['Avg. Symmetric Surface Distance'] <= 1e-10
    assert list(res.keys())[-4:] == EC.ADVANCED and len(res) == 17


@pytest.mark.parametrize('connectivity', [1, 2, 3])
@pytest.mark.parametrize('scenario', list(EC.SCENARIOS))
def test_surface_distances_against_scipy(dev, scenario, connectivity):
    a, b, spacing = EC.SCENARIOS[scenario]()
    _check_surface(a, b, spacing, connectivity, dev)


def test_surface_distances_beyond_one_tile(dev):
    a, b, spacing = EC.big_ellipsoids()
    _check_surface(a, b, spacing, 1, dev)


def test_surface_distances_long_thin_volume(dev):
    """A long y axis, rows shorter than a wave, masks far apart along y."""
    shape = (6, 700, 40)
    a = EC.ellipsoid(shape, (3, 200, 20), (2.5, 150, 12))
    b = EC.ellipsoid(shape, (2, 420, 18), (2.5, 200, 15))
    _check_surface(a, b, (2.0, 0.5, 1.0), 1, dev)


def test_nan_rules_without_a_launch(dev, monkeypatch):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.evaluation.evaluator import evaluate_case

    def boom(*a, **k):
        raise AssertionError("the surface op must not be called")
    monkeypatch.setattr(ops, 'surface_distances', boom)
    monkeypatch.setattr(ops, 'select_kth', boom)
    shape = (7, 9, 11)
    some = (np.random.default_rng(0).random(shape) < 0.3).astype(np.uint8)
    zeros, ones = np.zeros(shape, np.uint8), np.ones(shape, np.uint8)
    for t, r in ((zeros, some), (some, zeros), (ones, some), (some, ones)):
        for tt, rr in ((t, r), (torch.from_numpy(t).to(dev), torch.from_numpy(r).to(dev))):
            res = evaluate_case(tt, rr, [1, (1, 2)], advanced=True, advanced_metrics=EC.ADVANCED)
            for l in ('1', '(1, 2)'):
                assert len(res[l]) == 17
                for k in EC.ADVANCED:
                    assert math.isnan(res[l][k]), (l, k, res[l][k])


def test_advanced_input_checks(dev):
    import torch
    from multitalent_amd import _lib, ops
    from multitalent_amd.evaluation.evaluator import evaluate_case
    t, r = EC.golden_case(11)
    with pytest.raises(ValueError):
        evaluate_case(t.astype(np.int32) + 300, r, [1], advanced=True)
    with pytest.raises(ValueError):
        evaluate_case(t[0], r[0], [1], advanced=True)
    with pytest.raises(ValueError):
        evaluate_case(t, r, [1], advanced=True, connectivity=4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.surface_distances(torch.from_numpy(t), torch.from_numpy(r), np.ones(256, bool))
    with pytest.raises(ValueError):
        ops.sd_check_shape((2048, 1024, 1024))
    # the C entry point rejects D*H*W > INT32_MAX before any launch (nothing is read: the pointers are a 1-voxel volume's)
    one = torch.zeros(1, dtype=torch.uint8, device=dev)
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    member = np.ones(256, np.uint8)
    import ctypes as C
    rc = _lib.load().mt_surface_distances(one.data_ptr(), one.data_ptr(), 2048, 1024, 1024, member.ctypes.data_as(C.c_void_p), None, 1,
                                          buf.data_ptr(), 8, buf.data_ptr(), buf.data_ptr(), 64, None)
    assert rc == -1 and b"int32" in _lib.load().mt_last_error()          # MT_EINVAL


def _golden_pairs():
    return [EC.golden_case(c['seed'], c['absent']) for c in EC.GOLDEN_CASES]


def _check_against_golden(got, want, what):
    """key for key: the same metric names, NaN (null in the json) at the same places"""
    assert set(got.keys()) == set(want.keys()), what
    for k, w in want.items():
        g = got[k]
        if w is None:
            assert math.isnan(g), (what, k, g)
        elif k in EC.ADVANCED:
            tol = 1e-12 if k.startswith('Hausdorff') else 1e-10
            assert abs(g - w) <= tol * abs(w), (what, k, g, w)
        else:
            assert abs(g - w) <= 1e-12 * abs(w), (what, k, g, w)


def test_goldens_from_the_reference_evaluator(dev, tmp_path):
    from multitalent_amd.evaluation.evaluator import aggregate_scores
    gold = json.load(open(GOLDEN))
    labels = [tuple(l) if isinstance(l, list) else l for l in gold['labels']]
    assert labels == EC.GOLDEN_LABELS and gold['advanced_metrics'] == EC.ADVANCED
    pairs = _golden_pairs()
    for run in gold['runs']:
        conn = run['connectivity']
        for c, (t, r), want in zip(run['cases'], pairs, run['per_case']):
            got = aggregate_scores([(t, r)], labels=labels, advanced=True, advanced_metrics=EC.ADVANCED, voxel_spacing=c['spacing'],
                                   connectivity=conn)['all'][0]
            for l in labels:
                _check_against_golden(got[str(l)], want[str(l)], (c['name'], l, conn))
        jf = str(tmp_path / ('summary_%d.json' % conn))
        got = aggregate_scores(pairs, labels=labels, json_output_file=jf, json_name='golden', json_task='T', advanced=True,
                               advanced_metrics=EC.ADVANCED, voxel_spacing=run['joint_spacing'], connectivity=conn)
        assert len(got['all']) == len(run['joint']['all'])
        for i, want in enumerate(run['joint']['all']):
            for l in labels:
                _check_against_golden(got['all'][i][str(l)], want[str(l)], ('joint', i, l, conn))
        assert set(got['mean'].keys()) == set(run['joint']['mean'].keys())
        for l in labels:
            _check_against_golden(got['mean'][str(l)], run['joint']['mean'][str(l)], ('mean', l, conn))
        summary = json.load(open(jf))
        assert sorted(summary.keys()) == run['summary_keys'] and sorted(summary['results'].keys()) == run['summary_results_keys']
        assert summary['name'] == 'golden' and summary['task'] == 'T' and len(summary['id']) == 12


def test_evaluate_folder(dev, tmp_path):
    from multitalent_amd.evaluation.evaluator import aggregate_scores, evaluate_folder, main
    from multitalent_amd.utilities import nifti_io
    gt, pred = tmp_path / 'gt', tmp_path / 'pred'
    gt.mkdir()
    pred.mkdir()
    spacing_xyz = (0.75, 1.25, 3.0)                                 # nifti_io: (x, y, z); exact in the file's float32 pixdim
    pairs = _golden_pairs()[:3]
    for i, (t, r) in enumerate(pairs):
        nifti_io.write_image(t, str(pred / ('c%d.nii.gz' % i)), spacing_xyz)
        nifti_io.write_image(r, str(gt / ('c%d.nii.gz' % i)), (1.0, 1.0, 1.0))      # the TEST file's spacing is the one used
    labels = EC.GOLDEN_LABELS
    res = evaluate_folder(str(gt), str(pred), labels, advanced=True, advanced_metrics=EC.ADVANCED)
    assert os.path.isfile(str(pred / 'summary.json'))
    summary = json.load(open(str(pred / 'summary.json')))['results']
    arr = aggregate_scores(pairs, labels=labels, advanced=True, advanced_metrics=EC.ADVANCED, voxel_spacing=spacing_xyz[::-1])
    wrong = aggregate_scores(pairs, labels=labels, advanced=True, advanced_metrics=EC.ADVANCED, voxel_spacing=spacing_xyz)
    for l in labels:
        _same_metrics(res['mean'][str(l)], arr['mean'][str(l)])
        for k, v in arr['mean'][str(l)].items():
            s = summary['mean'][str(l)][k]
            assert (math.isnan(v) and math.isnan(s)) or s == v
    assert res['mean']['1']['Hausdorff Distance 95'] != wrong['mean']['1']['Hausdorff Distance 95']      # a z / x mix-up shows
    assert res['all'][0]['test'] == str(pred / 'c0.nii.gz') and res['all'][0]['reference'] == str(gt / 'c0.nii.gz')
    # the command line: default metrics only, then with --advanced (the reference's default advanced metric)
    out = main(['-ref', str(gt), '-pred', str(pred), '-l', '1', '2', '3'])
    assert len(out['mean']['1']) == 13
    out = main(['-ref', str(gt), '-pred', str(pred), '-l', '1', '2', '3', '--advanced'])
    assert list(out['mean']['1'].keys())[-1] == 'Hausdorff Distance 95' and len(out['mean']['1']) == 14
    assert out['mean']['1']['Hausdorff Distance 95'] == res['mean']['1']['Hausdorff Distance 95']


def test_select_kth(dev):
    import torch
    from multitalent_amd import ops
    rng = np.random.default_rng(2)
    for n in (1, 2, 63, 1000, 300001):
        x = np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-3, 4, n)
        x[rng.random(n) < 0.2] = 0.0
        x[rng.random(n) < 0.2] = 2.5                                # many ties
        ranks = sorted({0, n - 1, n // 2, n // 3, (19 * (n - 1)) // 20})
        got = ops.select_kth(torch.from_numpy(x).to(dev), ranks).cpu().numpy()
        assert np.array_equal(got, np.sort(x)[ranks]), n
    with pytest.raises(ValueError):
        ops.select_kth(torch.zeros(4, dtype=torch.float64, device=dev), [4])


def _f64_value_sets(rng, n):
    """Non-negative float64 inputs for the grouped radix select (8 passes of 8 bits on the uint64 key)."""
    tiny = np.nextafter(1.0, 2.0)
    return {'decades': np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-3, 4, n),          # seven decades
            'equal': np.full(n, 3.5),                                         # every rank in one group through all eight passes
            'last_bit': np.where(rng.random(n) < 0.5, 1.0, tiny),             # the groups split in pass 7 only
            'special': rng.choice(np.array([0.0, 5e-324, 1e-310, 1.0, np.inf]), n)}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 8191, 8192, 8193, 300001])
def test_select_kth_is_the_sorted_element(dev, n):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.experiment_planning.DatasetAnalyzer import _stat_ranks
    ranks = _stat_ranks(n)
    assert len(ranks) == 8
    sets = _f64_value_sets(np.random.default_rng(n), n)
    for name, x in sets.items():
        assert x.dtype == np.float64 and not np.signbit(x).any()
        xd = torch.from_numpy(x).to(dev)
        got = ops.select_kth(xd, ranks).cpu().numpy()
        again = ops.select_kth(xd, ranks).cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, np.sort(x)[ranks]), (name, n, got)
        assert got.tobytes() == again.tobytes()
    some = [n - 1, 0, n // 3]                                                # fewer ranks, in any order
    got = ops.select_kth(torch.from_numpy(sets['decades']).to(dev), some).cpu().numpy()
    assert np.array_equal(got, np.sort(sets['decades'])[some])


def test_select_kth_orders_signed_doubles(dev):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.experiment_planning.DatasetAnalyzer import _stat_ranks
    rng = np.random.default_rng(5)
    n = 8193
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    special = rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324, np.inf, -np.inf, 1.0, -1.0]), n)
    pick = rng.random(n) < 0.3
    x[pick] = special[pick]
    xd, srt = torch.from_numpy(x).to(dev), np.sort(x)
    ranks = _stat_ranks(n)
    got, want = ops.select_kth(xd, ranks).cpu().numpy(), srt[ranks]
    assert (want < 0).any() and np.array_equal(got, want)
    assert got[want != 0].tobytes() == want[want != 0].tobytes()
    # np.sort leaves the order of -0.0 and +0.0 open; the key puts every -0.0 before every +0.0: the bit patterns at the edges
    zeros = np.flatnonzero(srt == 0)
    nneg = int((np.signbit(x) & (x == 0)).sum())
    assert 0 < nneg < len(zeros)
    edge = [int(zeros[0]), int(zeros[nneg - 1]), int(zeros[nneg]), int(zeros[-1])]
    got = ops.select_kth(xd, edge).cpu().numpy()
    assert got.view(np.uint64).tolist() == [1 << 63, 1 << 63, 0, 0]


def test_select_kth_on_an_8_byte_aligned_view(dev):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.experiment_planning.DatasetAnalyzer import _stat_ranks
    rng = np.random.default_rng(7)
    for n in (1, 2, 5, 8193):
        full = np.abs(rng.standard_normal(n + 4)) * 100.0 + 1.0
        full[0] = 0.0
        full[n + 1:] = 1e9                                                   # neighbours that would change every rank
        view = torch.from_numpy(full).to(dev)[1:1 + n]
        assert view.data_ptr() % 16 == 8
        ranks = _stat_ranks(n)
        assert np.array_equal(ops.select_kth(view, ranks).cpu().numpy(), np.sort(full[1:1 + n])[ranks])
