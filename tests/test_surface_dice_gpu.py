"""Normalized surface Dice on the device.

The kernel alone (`mt_sd_count_within` through ops.sd_count_within) against numpy, exact: integer counts of fp64 comparisons.
Sizes: 1, 2, 63, 64, 65 (below, at and above one wave of pairs), 4099 (several workgroups, odd) and one round of the grid-stride
loop + 5; at each the first segment is empty, the whole array, odd and even; the array starts 0 and 8 bytes past a 16-byte
boundary, so both segments meet both alignments; 1, 3 and 8 tolerances.  The values hold the tolerance itself, its two
neighbours in float64, 0, +inf and subnormals.  The counts lie between poisoned guard words.

The metric against tests/golden/surface_dice.json (tools/oracle_gen/make_golden_surface_dice.py: the real reference's
normalized_surface_dice over the scipy restatement of medpy's distances; UNPINNED against medpy itself):
  * the value equals the golden to 1e-12 (absolute; the value lies in [0, 1]);
  * the integer counts equal the restatement's except for at most `exempt` distances per direction: restated distances within
    1e-12 (relative) of the tolerance, where a device distance that differs from scipy's in the last bits may fall on the other
    side.  With unit spacing (squared distances are integers and both sides take the correctly rounded root: 1.0 and 2.0 are exact
    ties, 1.25 and 2.6 have none) and at tolerance 0 nothing is exempt: those pin the `<=`.  The generator asserts that `exempt`
    stays below 1e-3 of a case's border voxels; in the committed golden it is 0 everywhere."""
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import evaluation_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
NSD = "Normalized Surface Dice"
POISON = 0x5a5a5a5a5a5a5a5a
GUARD = 4
V = 1.5                                                          # the tolerance that is a value of the array
SPECIAL = np.array([V, np.nextafter(V, 0.0), np.nextafter(V, 4.0), 0.0, np.inf, 5e-324, 1e-310, 0.75, 3.0])
TOLS = {1: [[0.0], [V], [np.inf]],
        3: [[0.0, V, np.inf]],
        8: [[0.0, V, np.inf, np.nextafter(V, 0.0), np.nextafter(V, 4.0), 5e-324, 0.75, 1e300]]}


def _grid_round(dev):
    """the elements one round of the grid-stride loop covers: 8 workgroups per CU (mt_stream_cap), 256 threads, 2 doubles each"""
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count * 8 * 256 * 2


def _counts(x, n_tr, tols):
    return np.array([[int((seg <= t).sum()) for t in tols] for seg in (x[:n_tr], x[n_tr:])], dtype=np.int64)


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 4099, 'round+5'])
def test_count_within_against_numpy(dev, n):
    import torch
    from multitalent_amd import ops
    n = _grid_round(dev) + 5 if n == 'round+5' else n
    rng = np.random.default_rng(n)
    host = rng.random(n + 1) * 3.0
    pick = rng.random(n + 1) < 0.6
    host[pick] = rng.choice(SPECIAL, int(pick.sum()))
    full = torch.from_numpy(host).to(dev)
    launches = 0
    for off in (0, 1):
        x = full[off:off + n]
        assert x.data_ptr() % 16 == 8 * off
        xh = host[off:off + n]
        for n_tr in sorted({0, n, 1, min(n, 2), n // 2, min(n, n // 2 + 1)}):
            for T, sets in TOLS.items():
                tols = sets[launches % len(sets)]
                buf = torch.full((2 * GUARD + 2 * T,), POISON, dtype=torch.int64, device=dev)
                out = ops.sd_count_within(x, n_tr, n - n_tr, tols, out=buf[GUARD:GUARD + 2 * T])
                launches += 1
                got = buf.cpu().numpy()
                assert out.shape == (2, T) and out.data_ptr() == buf.data_ptr() + 8 * GUARD
                assert (got[:GUARD] == POISON).all() and (got[GUARD + 2 * T:] == POISON).all(), (n, off, n_tr, T)
                assert np.array_equal(got[GUARD:GUARD + 2 * T].reshape(2, T), _counts(xh, n_tr, tols)), (n, off, n_tr, T, tols)
                again = ops.sd_count_within(x, n_tr, n - n_tr, tols).cpu().numpy()                 # a fresh output, second run
                assert np.array_equal(again, got[GUARD:GUARD + 2 * T].reshape(2, T))
    assert launches == 2 * 3 * len({0, n, 1, min(n, 2), n // 2, min(n, n // 2 + 1)})


def test_count_within_refusals_launch_nothing(dev):
    import ctypes as C
    import torch
    from multitalent_amd import _lib, ops
    x = torch.zeros(16, dtype=torch.float64, device=dev)
    buf = torch.full((16,), POISON, dtype=torch.int64, device=dev)
    for n_tr, n_rt, tols in ((8, 8, [float('nan')]), (8, 8, [1.0, -1e-300]), (8, 8, []), (8, 8, [1.0] * 9), (0, 0, [1.0]),
                             (-1, 8, [1.0]), (8, -2, [1.0]), (9, 8, [1.0])):
        with pytest.raises(ValueError, match="sd_count_within"):
            ops.sd_count_within(x, n_tr, n_rt, tols, out=buf[:2 * max(1, len(tols))] if len(tols) <= 8 else None)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream

    def call(sds, n_tr, n_rt, tols, T, out):
        arr = (C.c_double * max(1, len(tols)))(*tols)
        return lib.mt_sd_count_within(sds, n_tr, n_rt, C.cast(arr, C.c_void_p) if tols is not None else None, T, out, stream)
    for args in ((x.data_ptr(), 8, 8, [1.0], 0, buf.data_ptr()), (x.data_ptr(), 8, 8, [1.0] * 9, 9, buf.data_ptr()),
                 (x.data_ptr(), 0, 0, [1.0], 1, buf.data_ptr()), (x.data_ptr(), -1, 8, [1.0], 1, buf.data_ptr()),
                 (x.data_ptr(), 8, -1, [1.0], 1, buf.data_ptr()), (x.data_ptr(), 8, 8, [float('nan')], 1, buf.data_ptr()),
                 (x.data_ptr(), 8, 8, [0.5, -1.0], 2, buf.data_ptr()), (None, 8, 8, [1.0], 1, buf.data_ptr()),
                 (x.data_ptr(), 8, 8, [1.0], 1, None), (x.data_ptr() + 4, 4, 4, [1.0], 1, buf.data_ptr())):
        assert call(*args) == -1 and b"sd_count_within" in lib.mt_last_error(), args[1:5]           # MT_EINVAL
    assert lib.mt_sd_count_within(x.data_ptr(), 8, 8, None, 1, buf.data_ptr(), stream) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == POISON).all()                   # not even zeroed: nothing reached the stream
    assert ops.sd_count_within(x, 8, 8, [0.0, float('inf')], out=buf[:4]).cpu().tolist() == [[8, 8], [8, 8]]


GOLD = json.load(open(os.path.join(HERE, 'golden', 'surface_dice.json')))


def _to_dev(a, dev):
    import torch
    return torch.from_numpy(a.astype(np.uint8) * 5).to(dev)


@pytest.mark.parametrize('scenario', list(EC.SCENARIOS))
def test_metric_against_the_reference(dev, scenario):
    from multitalent_amd import ops
    from multitalent_amd.evaluation.evaluator import evaluate_case, nsd_from_counts
    assert GOLD['grid'] == list(EC.GRID) and GOLD['tolerances'] == [0.0, 1.0, 2.0, 1.25, 2.6, 1000.0] and GOLD['exempt_cap'] == 1e-3
    assert GOLD['spacings'] == [[1.0, 1.0, 1.0], [2.5, 0.8, 0.8]] and GOLD['connectivities'] == [1, 2, 3]
    cases = [c for c in GOLD['cases'] if c['scenario'] == scenario]
    assert len(cases) == 6
    a, b, _ = EC.SCENARIOS[scenario]()
    t, r = _to_dev(a, dev), _to_dev(b, dev)
    member = np.zeros(256, bool)
    member[5] = True
    worst = 0.0
    for c in cases:
        sp, conn = tuple(c['spacing']), c['connectivity']
        unit = sp == (1.0, 1.0, 1.0)
        sds, stats = ops.surface_distances(t, r, member, sp, conn, capacity=int(a.sum()) + int(b.sum()))
        st = stats.cpu().numpy()
        n_tr, n_rt = int(st[0]), int(st[3])
        assert (n_tr, n_rt) == (c['n_tr'], c['n_rt'])
        tols = [g['tolerance'] for g in c['by_tolerance']]
        counts = ops.sd_count_within(sds, n_tr, n_rt, tols).cpu().numpy()
        for k, g in enumerate(c['by_tolerance']):
            exempt = g['exempt']
            assert sum(exempt) <= GOLD['exempt_cap'] * (n_tr + n_rt)
            if unit or g['tolerance'] == 0:
                assert exempt == [0, 0]
            c_tr, c_rt = int(counts[0, k]), int(counts[1, k])
            assert abs(c_tr - g['c_tr']) <= exempt[0] and abs(c_rt - g['c_rt']) <= exempt[1], (scenario, conn, sp, g, c_tr, c_rt)
            res = evaluate_case(t, r, [5], advanced=True, advanced_metrics=[NSD], voxel_spacing=sp, connectivity=conn,
                                nsd_threshold=g['tolerance'])['5']
            assert list(res.keys())[-1] == NSD and len(res) == 14
            assert res[NSD] == nsd_from_counts(c_tr, n_tr, c_rt, n_rt)                          # one path
            worst = max(worst, abs(res[NSD] - g['value']))
            assert abs(res[NSD] - g['value']) <= 1e-12, (scenario, conn, sp, g, res[NSD])
        assert counts[:, -1].tolist() == [n_tr, n_rt]                                           # beyond the largest distance
    print("%s: worst |value - golden| = %.3g" % (scenario, worst))


def test_one_more_launch_per_entry_and_nothing_else_moves(dev, monkeypatch):
    """With the new name: one surface pass and one count per entry, the other metrics bit for bit what they are without it.
    Without it: no count launch, and the dicts of the parent commit (the goldens of the real reference's evaluator)."""
    from multitalent_amd import ops
    from multitalent_amd.evaluation import evaluator as E
    calls = {'sd': 0, 'count': 0}
    real_sd, real_count = ops.surface_distances, ops.sd_count_within
    monkeypatch.setattr(ops, 'surface_distances', lambda *a, **k: calls.__setitem__('sd', calls['sd'] + 1) or real_sd(*a, **k))
    monkeypatch.setattr(ops, 'sd_count_within', lambda *a, **k: calls.__setitem__('count', calls['count'] + 1) or real_count(*a, **k))
    gold = json.load(open(os.path.join(HERE, 'golden', 'evaluation.json')))
    labels = [tuple(l) if isinstance(l, list) else l for l in gold['labels']]
    run = [r for r in gold['runs'] if r['connectivity'] == 1][0]
    for c, want in zip(run['cases'], run['per_case']):
        t, r = EC.golden_case(c['seed'], c['absent'])
        calls.update(sd=0, count=0)
        got = E.evaluate_case(t, r, labels, advanced=True, advanced_metrics=EC.ADVANCED, voxel_spacing=c['spacing'], connectivity=1)
        present = sum(1 for l in labels if not math.isnan(got[str(l)]['Hausdorff Distance']))
        assert calls == {'sd': present, 'count': 0}
        for l in labels:
            assert set(got[str(l)].keys()) == set(want[str(l)].keys()) and len(got[str(l)]) == 17
            for k, w in want[str(l)].items():
                g = got[str(l)][k]
                if w is None:
                    assert math.isnan(g), (c['name'], l, k, g)
                else:
                    tol = 1e-10 if k.startswith('Avg.') else 1e-12          # the bounds of tests/test_evaluation_gpu.py
                    assert abs(g - w) <= tol * abs(w), (c['name'], l, k, g, w)
        calls.update(sd=0, count=0)
        both = E.evaluate_case(t, r, labels, advanced=True, advanced_metrics=EC.ADVANCED + [NSD], voxel_spacing=c['spacing'],
                               connectivity=1, nsd_threshold=2.0)
        assert calls == {'sd': present, 'count': present}
        for l in labels:
            assert list(both[str(l)].keys()) == list(got[str(l)].keys()) + [NSD]
            for k, g in got[str(l)].items():
                assert (math.isnan(g) and math.isnan(both[str(l)][k])) or g == both[str(l)][k], (l, k)
            assert math.isnan(both[str(l)][NSD]) == math.isnan(got[str(l)]['Hausdorff Distance'])
    assert both['test'] is None and both['reference'] is None


def test_nan_rules_without_a_launch(dev, monkeypatch):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.evaluation.evaluator import evaluate_case
    from multitalent_amd.evaluation.surface_dice import normalized_surface_dice

    def boom(*a, **k):
        raise AssertionError("no surface launch is expected")
    monkeypatch.setattr(ops, 'surface_distances', boom)
    monkeypatch.setattr(ops, 'sd_count_within', boom)
    shape = (7, 9, 11)
    some = (np.random.default_rng(0).random(shape) < 0.3).astype(np.uint8)
    zeros, ones = np.zeros(shape, np.uint8), np.ones(shape, np.uint8)
    for t, r in ((zeros, some), (some, zeros), (ones, some), (some, ones)):
        for tt, rr in ((t, r), (torch.from_numpy(t).to(dev), torch.from_numpy(r).to(dev))):
            res = evaluate_case(tt, rr, [1, (1, 2)], advanced=True, advanced_metrics=[NSD], nsd_threshold=1.0)
            assert math.isnan(res['1'][NSD]) and math.isnan(res['(1, 2)'][NSD]) and len(res['1']) == 14
            assert math.isnan(normalized_surface_dice(tt, rr, 1.0))


def test_thresholds_per_label_wrapper_and_symmetry(dev):
    import torch
    from multitalent_amd.evaluation import evaluator as E
    from multitalent_amd.evaluation.surface_dice import normalized_surface_dice
    t, r = EC.golden_case(11)
    sp = (2.5, 0.8, 0.8)
    kw = dict(advanced=True, advanced_metrics=[NSD], voxel_spacing=sp, connectivity=2)
    per = E.evaluate_case(t, r, [1, (1, 2)], nsd_threshold={'1': 1.0, '(1, 2)': 3.0}, **kw)
    one = E.evaluate_case(t, r, [1, (1, 2)], nsd_threshold=1.0, **kw)
    three = E.evaluate_case(t, r, [1, (1, 2)], nsd_threshold=3.0, **kw)
    assert per['1'][NSD] == one['1'][NSD] and per['(1, 2)'][NSD] == three['(1, 2)'][NSD]
    assert 0.0 < one['(1, 2)'][NSD] < three['(1, 2)'][NSD] < 1.0
    agg = E.aggregate_scores([(t, r), (r, t)], labels=[1, (1, 2)], nsd_threshold={'1': 1.0, '(1, 2)': 3.0}, **kw)
    assert agg['all'][0]['1'][NSD] == per['1'][NSD] and abs(agg['mean']['(1, 2)'][NSD] - per['(1, 2)'][NSD]) <= 1e-15
    # the wrapper: non-zero is the mask, for numpy and device inputs of any integer or bool type
    a, b = np.isin(t, (1, 2)), np.isin(r, (1, 2))
    want = three['(1, 2)'][NSD]
    assert normalized_surface_dice(a, b, 3.0, sp, 2) == want
    assert normalized_surface_dice(a.astype(np.int64) * 700, b.astype(np.int16) * -3, 3.0, spacing=sp, connectivity=2) == want
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert normalized_surface_dice(ad, bd, 3.0, sp, 2) == want
    assert normalized_surface_dice(ad.to(torch.int32) * 9, bd.to(torch.uint8), 3.0, sp, 2) == want
    for thr in (0.0, 1.0, 3.0):
        for conn in (1, 3):
            ab, ba = normalized_surface_dice(a, b, thr, sp, conn), normalized_surface_dice(b, a, thr, sp, conn)
            assert abs(ab - ba) <= 1e-15, (thr, conn, ab, ba)
    assert normalized_surface_dice(a, a, 0.0) == 2.0 / (2.0 + 1e-8)            # spacing None = 1 mm; every distance is 0


def test_command_line_nsd(dev, tmp_path):
    from multitalent_amd.evaluation.evaluator import evaluate_folder, main
    from multitalent_amd.utilities import nifti_io
    gt, pred = tmp_path / 'gt', tmp_path / 'pred'
    gt.mkdir()
    pred.mkdir()
    for i, c in enumerate(EC.GOLDEN_CASES[:2]):
        t, r = EC.golden_case(c['seed'], c['absent'])
        nifti_io.write_image(t, str(pred / ('c%d.nii.gz' % i)), (0.75, 1.25, 3.0))
        nifti_io.write_image(r, str(gt / ('c%d.nii.gz' % i)), (0.75, 1.25, 3.0))
    out = main(['-ref', str(gt), '-pred', str(pred), '-l', '1', '2', '--nsd', '2.5'])
    assert list(out['mean']['1'].keys())[-1] == NSD and len(out['mean']['1']) == 14
    adv = main(['-ref', str(gt), '-pred', str(pred), '-l', '1', '2', '--advanced', '--nsd', '2.5'])
    assert list(adv['mean']['1'].keys())[-2:] == ['Hausdorff Distance 95', NSD]
    want = evaluate_folder(str(gt), str(pred), [1, 2], advanced=True, advanced_metrics=[NSD], nsd_threshold=2.5)
    assert out['mean']['1'][NSD] == adv['mean']['1'][NSD] == want['mean']['1'][NSD]
    assert json.load(open(str(pred / 'summary.json')))['results']['mean']['2'][NSD] == want['mean']['2'][NSD]
    assert len(main(['-ref', str(gt), '-pred', str(pred), '-l', '1'])['mean']['1']) == 13
