"""The resize unit without a GPU: the float64 restatement (tests/resampling_cases.py) against scipy.ndimage.zoom / map_coordinates
themselves; csrc/resize_line.h as a stand-alone host program under the address and undefined-behaviour sanitizers against the
restatement; the new ABI entries; the preprocessor classes and the v2.3 planner; the refusals that need no device."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resampling_cases as RC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9                         # of the input range


def _range(x):
    return max(float(np.ptp(x)), 1.0)


# ---- the restatement against scipy ---------------------------------------------------------------------------------------------------
def test_line_cases_cover_every_tap_index():
    lengths = sorted(set(n for n, _ in RC.LINE_CASES))
    assert lengths == [1, 2, 3, 4, 5, 33]
    for n in lengths:
        bases = set(RC.tap_base3(o, n, m) for k, m in RC.LINE_CASES if k == n and m != n for o in range(m))
        assert bases == set(range(-2, n - 1)), (n, sorted(bases))            # first tap -2 .. n - 2: taps -2 .. n + 1
    assert any(m > 4 * n for n, m in RC.LINE_CASES) and any(n > 2 * m for n, m in RC.LINE_CASES) and any(n == m for n, m in RC.LINE_CASES)
    assert min(float(RC.coord(0, n, m)) for n, m in RC.LINE_CASES) < -0.48


@pytest.mark.parametrize('order', RC.ORDERS)
def test_restatement_equals_scipy_on_lines(order):
    worst = 0.0
    for n, m in RC.LINE_CASES:
        x = RC.hu_line(n, 100 * n + m).astype(np.float64)
        got = RC.resize_line(x, m, order)
        zoomed = ndimage.zoom(x, m / n, order=order, mode='nearest', grid_mode=True)
        mapped = ndimage.map_coordinates(x, [RC.coord(np.arange(m), n, m)], order=order, mode='nearest')
        assert zoomed.shape == (m,)
        dev = max(np.abs(got - zoomed).max(), np.abs(got - mapped).max()) / _range(x)
        worst = max(worst, dev)
        assert dev <= TOL, (n, m, order, dev)
        if order == 0:
            assert np.array_equal(got, zoomed) and np.array_equal(got, mapped), (n, m)
    print('order %d: worst deviation from scipy %.3g of the range' % (order, worst))


def test_order_0_takes_scipys_neighbour_for_every_small_pair_of_extents():
    """floor(x + 0.5) of the coordinate formed as ((o + 0.5) * (in / out)) - 0.5, each operation rounded, is the element scipy takes,
    also where the coordinate lies exactly between two elements (in/out = 4/3: every third one)."""
    total = ties = 0
    for n in range(1, 70):
        x = np.arange(n, dtype=np.float64)
        for m in range(1, 90):
            if m == n:
                continue
            c = RC.coord(np.arange(m), n, m)
            mine = np.clip(np.floor(c + 0.5), 0, n - 1)
            assert np.array_equal(mine, ndimage.zoom(x, m / n, order=0, mode='nearest', grid_mode=True)), (n, m)
            assert np.array_equal(mine, ndimage.map_coordinates(x, [c], order=0, mode='nearest')), (n, m)
            total += m
            ties += int((np.abs(c + 0.5 - np.round(c + 0.5)) < 1e-9).sum())
    assert total > 270000 and ties > 4900
    assert [RC.taps(0, o, 24, 18)[0][0] for o in range(18)] == [int(v) for v in ndimage.zoom(np.arange(24.0), 18 / 24, order=0, mode='nearest',
                                                                                           grid_mode=True)]


def test_extension_is_the_coefficient_of_the_padded_line():
    """c[-m] and c[n-1+m] from the stored coefficients alone equal what scipy's filter gives on a line padded with its edge values."""
    for n in (2, 3, 4, 5, 33):
        x = RC.hu_line(n, 7 * n).astype(np.float64)
        c = RC.prefilter_line(x)
        ref = ndimage.spline_filter1d(np.pad(x, 40, mode='edge'), order=3, mode='mirror')[40 - 2:40 + n + 2]
        assert np.abs(c - ref[2:-2]).max() <= TOL * _range(x)
        got = [RC.extend(c[0], c[1], 2), RC.extend(c[0], c[1], 1), RC.extend(c[-1], c[-2], 1), RC.extend(c[-1], c[-2], 2)]
        assert np.abs(np.array(got) - np.concatenate([ref[:2], ref[-2:]])).max() <= TOL * _range(x), n


VOLUME_SCIPY = [((9, 20, 18), (13, 27, 25)), ((5, 12, 12), (10, 24, 24)), ((7, 24, 22), (14, 18, 17)), ((24, 26, 22), (13, 15, 14)),
                ((1, 2, 3), (4, 7, 9))]


@pytest.mark.parametrize('order', RC.ORDERS)
def test_restatement_equals_scipy_zoom_in_3d(order):
    for i, (shape, new) in enumerate(VOLUME_SCIPY):
        v = RC.hu_volume(shape, 40 + i).astype(np.float64)
        got = RC.resize_data(v, new, (order,) * 3, store=np.float64)[0]
        ref = ndimage.zoom(v[0], [b / a for a, b in zip(shape, new)], order=order, mode='nearest', grid_mode=True)
        assert np.abs(got - ref).max() <= TOL * _range(v), (shape, new, order)


@pytest.mark.parametrize('ax', [0, 1, 2])
def test_restatement_equals_the_two_stage_branch(ax):
    """Per slice across `ax` at order 3, then map_coordinates(order_z) along it: orders (3, 3), (3, 1), (3, 0), (1, 0)."""
    shape, new = [20, 18, 22], [27, 25, 17]
    shape[ax], new[ax] = 7, 12
    v = RC.hu_volume(shape, 50 + ax).astype(np.float64)
    mid = [shape[a] if a == ax else new[a] for a in range(3)]
    for order, order_z in ((3, 3), (3, 1), (3, 0), (1, 0)):
        slices = [ndimage.zoom(np.take(v[0], s, axis=ax), [new[a] / shape[a] for a in range(3) if a != ax], order=order, mode='nearest',
                               grid_mode=True) for s in range(shape[ax])]
        ref1 = np.stack(slices, ax)
        grid = np.mgrid[:new[0], :new[1], :new[2]].astype(np.float64)
        coords = [RC.coord(grid[a], mid[a], new[a]) for a in range(3)]
        ref = ndimage.map_coordinates(ref1, coords, order=order_z, mode='nearest')
        got1 = RC.resize_data(v, mid, tuple(0 if a == ax else order for a in range(3)), store=np.float64)
        assert np.abs(got1[0] - ref1).max() <= TOL * _range(v)
        got = RC.resize_data(got1, new, tuple(order_z if a == ax else 0 for a in range(3)), store=np.float64)[0]
        assert np.abs(got - ref).max() <= TOL * _range(v), (ax, order, order_z)


def test_label_restatement_equals_the_reference_rules():
    """In plane: resize_segmentation(order 1), `>= 0.5`, ascending labels.  The z pass: np.round(...) > 0.5 per label."""
    seg = RC.blocky_labels((7, 12, 11), 3)
    new = (7, 17, 9)
    got = RC.resize_labels(seg, new)[0]
    ref = np.zeros(new)
    for c in np.unique(seg):
        w = np.stack([ndimage.zoom((seg[0, s] == c).astype(float), [17 / 12, 9 / 11], order=1, mode='nearest', grid_mode=True) for s in range(7)])
        ref[w >= 0.5] = c
    fragile = np.zeros(new, dtype=bool)
    for c in np.unique(seg):
        w = np.stack([ndimage.zoom((seg[0, s] == c).astype(float), [17 / 12, 9 / 11], order=1, mode='nearest', grid_mode=True) for s in range(7)])
        fragile |= np.abs(w - 0.5) < 1e-9
    assert np.array_equal(got[~fragile], ref[~fragile]) and fragile.mean() < 0.1
    for n_out in (14, 4, 21):                       # 14 = 2 x 7: weights of exactly one half occur, and there no label wins
        gotz = RC.resize_labels_axis(ref[None], 0, n_out)[0]
        grid = np.mgrid[:n_out, :17, :9].astype(np.float64)
        coords = [RC.coord(grid[0], 7, n_out), grid[1], grid[2]]
        refz = np.zeros((n_out, 17, 9))
        for c in np.unique(ref):
            refz[np.round(ndimage.map_coordinates((ref == c).astype(float), coords, order=1, mode='nearest')) > 0.5] = c
        assert np.array_equal(gotz, refz), n_out
    assert RC.label_vote([-1.0, 3.0], [0.5, 0.5], strict=True) == 0.0 and RC.label_vote([-1.0, 3.0], [0.5, 0.5], strict=False) == 3.0
    assert RC.label_vote([-1.0, -1.0], [0.25, 0.75], strict=True) == -1.0 and RC.label_vote([-1.0, 0.0], [0.5, 0.5], strict=False) == 0.0


# ---- the header as a host program ----------------------------------------------------------------------------------------------------
VOTES = [(0, [-1.0, 3.0], [0.5, 0.5]), (1, [-1.0, 3.0], [0.5, 0.5]), (1, [-1.0, -1.0], [0.25, 0.75]), (0, [-1.0, 0.0], [0.5, 0.5]),
         (0, [2.0, 1.0, 2.0, 0.0, 5.0, 5.0, 1.0, 0.0], [0.2, 0.1, 0.31, 0.09, 0.05, 0.05, 0.1, 0.1]),
         (1, [2.0, 1.0, -1.0, 0.0, 5.0, 5.0, 1.0, 0.0], [0.2, 0.4, -1.0, 0.1, -1.0, 0.05, 0.15, 0.1]),
         (0, [4.0], [1.0]), (1, [0.0, 7.0], [0.49, 0.51]), (1, [7.0, 0.0], [0.3, 0.7])]


def test_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'resize_line_host')
    subprocess.check_call(['/opt/rocm/bin/hipcc' if os.path.isfile('/opt/rocm/bin/hipcc') else 'hipcc', '--offload-arch=gfx950', '-O1', '-g',
                           '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                           '-I', os.path.join(ROOT, 'multitalent_amd', 'csrc'), os.path.join(ROOT, 'tests', 'resize_line_host.cpp'), '-o', exe])
    cases = [(n, m, order) for n, m in RC.LINE_CASES for order in RC.ORDERS]
    src, dst = str(tmp_path / 'cases.txt'), str(tmp_path / 'results.txt')
    with open(src, 'w') as f:
        for n, m, order in cases:
            f.write('S %d %d %d %s\n' % (n, m, order, ' '.join(repr(float(v)) for v in RC.hu_line(n, 100 * n + m))))
        for strict, lab, w in VOTES:
            f.write('L %d %d %s %s\n' % (strict, len(lab), ' '.join(repr(v) for v in lab), ' '.join(repr(v) for v in w)))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(dst).read().splitlines()
    pos = 0
    seen = set()
    for n, m, order in cases:
        x = RC.hu_line(n, 100 * n + m).astype(np.float64)
        c = RC.prefilter_line(x) if order == 3 and n != m else x
        tol = 1e-12 * _range(x)
        assert lines[pos][0] == 'C'
        assert np.abs(np.array(lines[pos].split()[1:], dtype=np.float64) - c).max() <= tol, (n, m, order)
        pos += 1
        for o in range(m):
            t = lines[pos].split(); pos += 1
            idx, w = RC.taps(order, o, n, m)
            nt = RC.ntaps(order, n, m)
            assert t[0] == 'T' and int(t[1]) == o and int(t[3]) == nt == len(idx)
            assert [int(v) for v in t[4:4 + nt]] == idx, (n, m, order, o)
            assert np.abs(np.array(t[4 + nt:], dtype=np.float64) - np.array(w)).max() <= 1e-14, (n, m, order, o)
            assert abs(sum(w) - 1.0) <= 1e-14
            if order == 3 and n != m:
                assert int(t[2]) == RC.tap_base3(o, n, m)
                seen.update((n, int(t[2]) + k) for k in range(4))
        assert lines[pos][0] == 'R'
        assert np.abs(np.array(lines[pos].split()[1:], dtype=np.float64) - RC.resize_line(x, m, order)).max() <= tol, (n, m, order)
        pos += 1
        if n > 1:
            e = np.array(lines[pos].split()[1:], dtype=np.float64); pos += 1
            want = [RC.extend(c[0], c[1], 1), RC.extend(c[0], c[1], 2), RC.extend(c[-1], c[-2], 1), RC.extend(c[-1], c[-2], 2)]
            assert np.abs(e - np.array(want)).max() <= tol
    for n in (1, 2, 3, 4, 5, 33):
        assert set(i for k, i in seen if k == n) == set(range(-2, n + 2)), n
    for strict, lab, w in VOTES:
        assert lines[pos].split() == ['V', '%.9g' % RC.label_vote(lab, w, bool(strict))], (strict, lab, w)
        pos += 1
    assert pos == len(lines)


# ---- ABI, classes, planner, refusals ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('mt_resize_prefilter3', 'mt_resize', 'mt_resize_labels', 'mt_resize_labels_axis')


def test_new_entries_are_in_header_library_and_signatures():
    from multitalent_amd import _lib
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mtseg.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(mt_[a-z0-9_]+)\s*\(', txt))
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.mt_abi_version() == 4                                       # entries are only added


def test_refusals_need_no_device():
    """Every refusal of the C entries comes before a launch: with MT_EINVAL and a message, on a machine without a device too."""
    import ctypes as C
    from multitalent_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    bad = [lambda: lib.mt_resize_prefilter3(None, p, 1, 2, 2, 2, 7, None), lambda: lib.mt_resize_prefilter3(p, None, 1, 2, 2, 2, 7, None),
           lambda: lib.mt_resize_prefilter3(p, p, 0, 2, 2, 2, 7, None), lambda: lib.mt_resize_prefilter3(p, p, 1, 2, -2, 2, 7, None),
           lambda: lib.mt_resize_prefilter3(p, p, 1, 2, 2, 2, 0, None), lambda: lib.mt_resize_prefilter3(p, p, 1, 2, 2, 2, 8, None),
           lambda: lib.mt_resize_prefilter3(p, p, 1 << 16, 1 << 15, 1, 1, 1, None),
           lambda: lib.mt_resize(None, 1, 2, 2, 2, p, 2, 2, 2, 1, 1, 1, None), lambda: lib.mt_resize(p, 1, 2, 2, 2, None, 2, 2, 2, 1, 1, 1, None),
           lambda: lib.mt_resize(p, 1, 2, 0, 2, p, 2, 2, 2, 1, 1, 1, None), lambda: lib.mt_resize(p, 1, 2, 2, 2, p, 2, 2, 0, 1, 1, 1, None),
           lambda: lib.mt_resize(p, 1, 2, 2, 2, p, 2, 2, 2, 2, 1, 1, None), lambda: lib.mt_resize(p, 1, 2, 2, 2, p, 2, 2, 2, 1, 5, 1, None),
           lambda: lib.mt_resize(p, 1, 2, 2, 2, p, 2, 2, 2, 1, 1, -1, None),
           lambda: lib.mt_resize(p, 1 << 16, 1 << 15, 1, 1, p, 1, 1, 1, 0, 0, 0, None),
           lambda: lib.mt_resize(p, 1, 1, 1, 1, p, 1 << 11, 1 << 10, 1 << 10, 0, 0, 0, None),
           lambda: lib.mt_resize_labels(None, 1, 2, 2, 2, p, 2, 2, 2, None), lambda: lib.mt_resize_labels(p, 1, 2, 2, 2, p, 2, -1, 2, None),
           lambda: lib.mt_resize_labels(p, 1, 1, 1, 1, p, 1 << 11, 1 << 10, 1 << 10, None),
           lambda: lib.mt_resize_labels_axis(p, 1, 2, 2, 2, 3, 4, p, None), lambda: lib.mt_resize_labels_axis(p, 1, 2, 2, 2, -1, 4, p, None),
           lambda: lib.mt_resize_labels_axis(p, 1, 2, 2, 2, 0, 0, p, None), lambda: lib.mt_resize_labels_axis(p, 1, 2, 2, 2, 0, 4, None, None),
           lambda: lib.mt_resize_labels_axis(p, 1, 2, 1 << 15, 1 << 15, 0, 4, p, None)]
    for i, call in enumerate(bad):
        assert call() == -1, i                                               # MT_EINVAL
        assert lib.mt_last_error(), i
    assert all(v == 0.0 for v in buf)


def test_classes_and_planner_are_importable(tmp_path):
    from multitalent_amd.experiment_planning.alternative_experiment_planning.experiment_planner_baseline_3DUNet_v23 import \
        ExperimentPlanner3D_v23
    from multitalent_amd.experiment_planning.experiment_planner_baseline_3DUNet_v21 import ExperimentPlanner3D_v21
    from multitalent_amd.experiment_planning.nnUNet_plan_and_preprocess import _find_planner
    from multitalent_amd.preprocessing import preprocessing as P
    from multitalent_amd.training.model_restore import recursive_find_python_class
    import multitalent_amd
    folder = [os.path.join(multitalent_amd.__path__[0], 'preprocessing')]
    for name in ('GenericPreprocessor', 'GenericPreprocessor_linearResampling', 'Preprocessor3DDifferentResampling'):
        cls = recursive_find_python_class(folder, name, 'multitalent_amd.preprocessing')
        assert cls is getattr(P, name) and issubclass(cls, P.GenericPreprocessor)
    assert P.PREPROCESSORS == ('GenericPreprocessor', 'GenericPreprocessor_linearResampling', 'Preprocessor3DDifferentResampling')
    lin = P.GenericPreprocessor_linearResampling({0: 'CT'}, {0: False}, [0, 1, 2], None)
    assert (lin.resample_order_data, lin.resample_order_seg, lin.resample_order_z_data, lin.resample_order_z_seg) == (1, 1, 0, 0)
    dif = P.Preprocessor3DDifferentResampling({0: 'CT'}, {0: False}, [0, 1, 2], None)
    assert (dif.resample_order_data, dif.resample_order_seg, dif.resample_order_z_data, dif.resample_order_z_seg) == (3, 1, 3, 1)
    gen = P.GenericPreprocessor({0: 'CT'}, {0: False}, [0, 1, 2], None)
    assert (gen.resample_order_data, gen.resample_order_seg) == (3, 1) and type(gen)._resample is P.GenericPreprocessor._resample
    # the planner: the reference's three attributes (experiment_planner_baseline_3DUNet_v23.py:25-28)
    assert _find_planner('ExperimentPlanner3D_v23') is ExperimentPlanner3D_v23 and issubclass(ExperimentPlanner3D_v23, ExperimentPlanner3D_v21)
    cropped, pre = str(tmp_path / 'cropped'), str(tmp_path / 'preprocessed')
    os.makedirs(cropped)
    with open(os.path.join(cropped, 'dataset_properties.pkl'), 'wb') as f:
        pickle.dump({'all_classes': [1]}, f)
    planner = ExperimentPlanner3D_v23(cropped, pre)
    assert planner.data_identifier == 'nnUNetData_plans_v2.3'
    assert planner.plans_fname == os.path.join(pre, 'nnUNetPlansv2.3_plans_3D.pkl')
    assert planner.preprocessor_name == 'Preprocessor3DDifferentResampling'


def test_python_refusals_without_a_device():
    import torch
    from multitalent_amd.preprocessing import device_preprocessing as dp
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dp.resample_data_or_seg(x, (5, 5, 5), False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dp.resample_patient(x, None, (1, 1, 1), (2, 2, 2))


def test_preprocess_patient_still_refuses_an_unknown_name():
    from multitalent_amd.training.network_training.nnUNetTrainer import nnUNetTrainer
    tr = nnUNetTrainer.__new__(nnUNetTrainer)
    for name in ('Preprocessor3DBetterResampling', 'PreprocessorFor2D', 'nonsense'):
        tr.plans = {'preprocessor_name': name}
        with pytest.raises(NotImplementedError, match='preprocessor %s is not on this path' % name):
            tr.preprocess_patient(['x.nii.gz'])
