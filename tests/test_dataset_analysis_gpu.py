"""The dataset fingerprint on the device: the kernels of csrc/analyze.hip and csrc/select.hip against numpy (bit for bit / `==`), `DatasetAnalyzer`
against the REAL reference's (tools/oracle_gen/make_golden_dataset_analysis.py -> golden/dataset_analysis.npz), and the chain offline
cropper -> analyzer -> GenericPreprocessor.run on files.
Bounds against the golden: mn and mx equal; an interpolated value within 2 x dev64 + 1 float32 ulp of the value; mean and sd within
2 x dev64 + 1e-6 x max(1, |value|) (the device takes the moments in double and rounds once).  dev64 is the reference's own recorded
deviation of that value from the same formula in float64."""
import ctypes as C
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataset_analysis.npz')
INTERP = ('median', 'percentile_99_5', 'percentile_00_5')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
def _make_seg(rs, shape, density):
    V = int(np.prod(shape))
    if density == 'last':
        seg = np.zeros(V, dtype=np.float32)
        seg[-1] = 3
    elif density == 0:
        seg = np.where(rs.rand(V) < 0.5, -1, 0).astype(np.float32)
    elif density == 1.0:
        seg = rs.randint(1, 4, V).astype(np.float32)
    else:
        seg = np.where(rs.rand(V) < density, rs.randint(1, 4, V), rs.randint(-1, 1, V)).astype(np.float32)
    return seg.reshape(shape)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (1, 1, 64), (1, 1, 65), (17, 33, 65), (64, 64, 64)])
def test_fg_sample_is_the_strided_numpy_selection(dev, shape):
    from multitalent_amd import ops
    rs = np.random.RandomState(sum(shape))
    for Cn in (1, 3):
        data = (rs.randn(Cn, *shape) * 300 - 100).astype(np.float32)
        dd = torch.from_numpy(data).to(dev)
        for density in (0, 1.0, 0.5, 0.003, 'last'):
            seg = _make_seg(rs, shape, density)
            sd = torch.from_numpy(seg).to(dev)
            index = ops.fg_sample_count(sd)
            n_want = int((seg > 0).sum())
            assert index.n == n_want and int(index.count.item()) == n_want
            for stride in (1, 7, 10):
                want = np.stack([data[c][seg > 0][::stride] for c in range(Cn)])
                out, n, nans = ops.fg_sample(dd, sd, stride, index=index)
                assert n == n_want and out.shape == want.shape and out.dtype == torch.float32
                assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (shape, Cn, density, stride)
                assert nans.cpu().tolist() == [0] * Cn
        assert ops.fg_sample(dd, sd, 10)[1] == n_want                       # without a prepared index


def test_fg_sample_float_predicate_nan_counts_slots_and_repeatability(dev):
    from multitalent_amd import ops
    rs = np.random.RandomState(3)
    shape = (17, 33, 65)
    V = int(np.prod(shape))
    seg = rs.choice(np.array([-1, 0, 0.5, 2, np.nan], dtype=np.float32), V).reshape(shape)       # 0.5 and 2 are selected
    data = rs.randn(3, *shape).astype(np.float32)
    fg = np.flatnonzero(seg.reshape(-1) > 0)
    assert 0 < len(fg) < V and np.isnan(seg).any()
    d1 = data[1].reshape(-1)
    nan_bits = np.array([0x7fc00001, 0xffc12345, 0x7f800001], dtype=np.uint32).view(np.float32)     # payloads must survive
    d1[fg[0]], d1[fg[10]], d1[fg[20]] = nan_bits        # sampled by stride 10 (ranks 0, 10, 20)
    d1[fg[5]] = np.nan                                  # in the foreground but not sampled by stride 10
    dd, sd = torch.from_numpy(data).to(dev), torch.from_numpy(seg).to(dev)
    for stride, n_nan in ((10, 3), (5, 4), (1, 4)):
        want = np.stack([data[c][seg > 0][::stride] for c in range(3)])
        out, n, nans = ops.fg_sample(dd, sd, stride)
        assert n == len(fg) and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
        assert nans.cpu().tolist() == [0, n_nan, 0]
    # a slot of a larger buffer: channel stride larger than m, neighbours untouched
    m = (len(fg) + 9) // 10
    buf = torch.full((3, 2 * m + 11), -7.0, device=dev)
    out, _, _ = ops.fg_sample(dd, sd, 10, out=buf, offset=5)
    want = np.stack([data[c][seg > 0][::10] for c in range(3)])
    host = buf.cpu().numpy()
    assert out.data_ptr() == buf.data_ptr() + 20 and np.array_equal(_bits(host[:, 5:5 + m]), _bits(want))
    assert (host[:, :5] == -7).all() and (host[:, 5 + m:] == -7).all()
    again = torch.full((3, 2 * m + 11), -7.0, device=dev)
    ops.fg_sample(dd, sd, 10, out=again, offset=5)
    assert torch.equal(buf.view(torch.int32), again.view(torch.int32))       # bit-equal from run to run
    with pytest.raises(ValueError, match="do not fit"):
        ops.fg_sample(dd, sd, 10, out=buf, offset=buf.shape[1] - m + 1)
    with pytest.raises(ValueError, match="stride"):
        ops.fg_sample(dd, sd, 0)
    with pytest.raises(ValueError, match="channels"):
        ops.fg_sample(torch.zeros((17, 4), device=dev), torch.zeros(4, device=dev), 10)


def test_fg_sample_over_more_units_than_scan_threads(dev):
    """301 units of 8192 voxels, the last one 5 voxels long: every thread of the scan's workgroup owns up to two units, and the
    threads beyond unit 300 none."""
    from multitalent_amd import ops
    rs = np.random.RandomState(11)
    V = 8192 * 300 + 5
    density = np.linspace(0.02, 0.9, V) * (np.arange(V) // 8192 % 7 != 3)    # rising along the volume, some units empty
    seg = np.where(rs.rand(V) < density, rs.randint(1, 4, V), rs.randint(-1, 1, V)).astype(np.float32).reshape(1, 1, V)
    seg[0, 0, -1] = 2
    data = rs.randn(2, 1, 1, V).astype(np.float32)
    dd, sd = torch.from_numpy(data).to(dev), torch.from_numpy(seg).to(dev)
    for stride in (10, 1):
        want = data[:, seg > 0][:, ::stride]
        out, n, nans = ops.fg_sample(dd, sd, stride)
        assert n == int((seg > 0).sum()) and np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and nans.cpu().tolist() == [0, 0]


# ---- select -------------------------------------------------------------------------------------------------------------------------
def _value_sets(rs, n):
    tiny = np.nextafter(np.float32(1), np.float32(2))
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf, 1.0, -1.0], dtype=np.float32)
    return {'hu': rs.randint(-1024, 3072, n).astype(np.float32),
            'normal': (rs.randn(n) * 175 + 63).astype(np.float32),
            'equal': np.full(n, -3.5, dtype=np.float32),
            'last_bit': np.where(rs.rand(n) < 0.5, np.float32(1), tiny).astype(np.float32) * np.float32(-1 if n % 2 else 1),
            'sign': np.where(rs.rand(n) < 0.5, np.float32(2.5), np.float32(-2.5)).astype(np.float32),
            'special': rs.choice(special, n)}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 8191, 8192, 8193, 1000003])
def test_select_kth_f32_is_the_sorted_element(dev, n):
    from multitalent_amd import ops
    from multitalent_amd.experiment_planning.DatasetAnalyzer import _stat_ranks
    ranks = _stat_ranks(n)
    assert len(ranks) == 8
    for name, x in _value_sets(np.random.RandomState(n), n).items():
        want = np.sort(x)[ranks]
        xd = torch.from_numpy(x).to(dev)
        got = ops.select_kth_f32(xd, ranks).cpu().numpy()
        again = ops.select_kth_f32(xd, ranks).cpu().numpy()
        assert got.dtype == np.float32 and (got == want).all(), (name, n, got, want)
        assert got.tobytes() == again.tobytes()
        assert np.isin(_bits(got), _bits(x)).all()                          # elements of x, bit for bit
    # fewer ranks, in any order
    x = _value_sets(np.random.RandomState(1), n)['normal']
    some = [n - 1, 0, n // 3]
    assert (ops.select_kth_f32(torch.from_numpy(x).to(dev), some).cpu().numpy() == np.sort(x)[some]).all()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_select_kth_f32_on_a_dword_aligned_view(dev, offset):
    from multitalent_amd import ops
    from multitalent_amd.experiment_planning.DatasetAnalyzer import _stat_ranks
    rs = np.random.RandomState(offset)
    for n in (1, 2, 5, 8193):
        full = rs.randint(-1024, 3072, n + offset + 3).astype(np.float32)
        full[:offset] = -5000
        full[offset + n:] = 9000                                             # neighbours that would change every rank
        view = torch.from_numpy(full).to(dev)[offset:offset + n]
        assert view.data_ptr() % 16 == 4 * offset
        ranks = _stat_ranks(n)
        assert (ops.select_kth_f32(view, ranks).cpu().numpy() == np.sort(full[offset:offset + n])[ranks]).all()


# ---- label presence -------------------------------------------------------------------------------------------------------------------
def test_label_presence_is_np_unique(dev):
    from multitalent_amd import ops
    rs = np.random.RandomState(4)
    for shape, labels in (((1, 1, 1), [0]), ((3, 5, 7), [-1, 0, 1]), ((17, 33, 65), [-1, 0, 5, 31, 32, 63, 64, 1000, 1022]),
                          ((40, 40, 41), [1022]), ((9, 9, 9), [-1])):
        seg = rs.choice(np.array(labels, dtype=np.float32), int(np.prod(shape))).reshape(shape)
        seg.reshape(-1)[:len(labels)] = labels
        got = ops.label_presence(torch.from_numpy(seg).to(dev))
        assert got == [int(i) for i in np.unique(seg)] == sorted(labels)
    seg = np.zeros((17, 33, 65), dtype=np.float32)
    sd = torch.from_numpy(seg).to(dev)
    assert ops.label_presence(sd[1:].contiguous().view(-1)[1:]) == [0]       # a dword-aligned view
    for bad in (0.5, 1023, np.nan, -2, np.inf):
        s = seg.copy()
        s[16, 32, 64] = bad
        with pytest.raises(ValueError, match="case liver_7"):
            ops.label_presence(torch.from_numpy(s).to(dev), "the segmentation of case liver_7")


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_before_any_launch(dev):
    from multitalent_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(16, device=dev)
    out = torch.zeros(8, device=dev)
    ws = torch.zeros(int(lib.mt_select_kth_f32_workspace(8)), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def select(n, ranks, ws_bytes=None):
        rk = (C.c_long * len(ranks))(*ranks)
        return lib.mt_select_kth_f32(p(x), n, C.cast(rk, C.c_void_p), len(ranks), p(out), p(ws), ws.numel() if ws_bytes is None else ws_bytes, None)

    assert select(16, [0, 15]) == 0
    assert select(0, [0]) == -1 and b"element count" in lib.mt_last_error()                # MT_EINVAL
    assert select(16, list(range(9))) == -1 and b"ranks" in lib.mt_last_error()
    assert select(16, [16]) == -1 and b"outside" in lib.mt_last_error()
    assert select(16, [-1]) == -1
    assert select(16, [0], ws_bytes=ws.numel() - 1) == -2                                   # MT_EWORKSPACE
    assert lib.mt_select_kth_f32_workspace(9) == 0 and lib.mt_select_kth_f32_workspace(0) == 0
    seg = torch.ones(20000, device=dev)
    need = int(lib.mt_fg_sample_workspace(20000))
    fws = torch.zeros(need, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    nan = torch.zeros(17, dtype=torch.int64, device=dev)
    fout = torch.zeros(20000, device=dev)
    assert need >= 4 * 3 and lib.mt_fg_sample_count(p(seg), 20000, p(cnt), p(fws), need, None) == 0
    assert lib.mt_fg_sample_count(p(seg), 20000, p(cnt), p(fws), need - 8, None) == -2
    assert lib.mt_fg_sample_count(p(seg), 2 ** 31, p(cnt), p(fws), need, None) == -1 and b"int32" in lib.mt_last_error()
    gather = lambda Cn, V, stride, wsb: lib.mt_fg_sample_gather(p(seg), Cn, V, p(seg), stride, p(fws), wsb, p(fout), 20000, p(nan), None)
    assert gather(1, 20000, 10, need) == 0
    assert gather(17, 20000, 10, need) == -1 and gather(1, 20000, 0, need) == -1 and gather(1, 2 ** 31, 10, need) == -1
    assert gather(1, 20000, 10, need - 8) == -2
    torch.cuda.synchronize()
    assert int(cnt.item()) == 20000 and torch.equal(fout[:2000], torch.ones(2000, device=dev)) and float(fout[2000]) == 0
    with pytest.raises(ValueError):
        ops.select_kth_f32(x, [])
    with pytest.raises(ValueError):
        ops.select_kth_f32(x, [16])
    with pytest.raises(ValueError):
        ops.select_kth_f32(x, list(range(9)))
    with pytest.raises(ValueError):
        ops.select_kth_f32(x[:0], [0])
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.select_kth_f32(torch.zeros(4), [0])


# ---- analyzer ---------------------------------------------------------------------------------------------------------------------------
def _golden_folder(z, folder):
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, 'dataset.json'), 'w') as f:
        f.write(str(z['dataset_json']))
    for name in z['names']:
        data, seg = z[name + '/data'], z[name + '/seg'].astype(np.float32)
        np.savez_compressed(os.path.join(folder, name + '.npz'), data=np.vstack((data, seg)))
        with open(os.path.join(folder, name + '.pkl'), 'wb') as f:
            pickle.dump({'original_size_of_raw_data': z[name + '/raw_size'], 'original_spacing': z[name + '/spacing'],
                         'size_after_cropping': tuple(int(i) for i in data.shape[1:])}, f)
    return folder


def _same(a, b):
    """Equality of nested results, NaN equal to NaN, types included."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a.keys()) == list(b.keys()) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    if isinstance(a, (float, np.floating)) and np.isnan(a):
        return bool(np.isnan(b))
    return a == b


def _check_against_golden(z, ip):
    keys = list(z['stat_keys'])
    assert list(ip.keys()) == [0, 1]
    for c in (0, 1):
        assert list(ip[c].keys()) == list(z['ip_keys']) and list(ip[c]['local_props'].keys()) == list(z['names'])
        rows = [ip[c]['local_props'][n] for n in z['names']] + [ip[c]]
        for i, row in enumerate(rows):
            if i < len(z['names']):
                assert list(row.keys()) == keys
            for j, k in enumerate(keys):
                got, want, dev64 = row[k], z['stats'][c, i, j], float(z['dev64'][c, i, j])
                assert type(got).__name__ == str(z['types'][c, i, j]), (c, i, k, type(got))
                if np.isnan(want):
                    assert np.isnan(got)
                    continue
                if k in ('mn', 'mx'):
                    bound = 0.0
                elif k in INTERP:
                    bound = 2 * dev64 + float(np.spacing(np.abs(np.float32(want))))
                else:
                    bound = 2 * dev64 + 1e-6 * max(1.0, abs(float(want)))
                d = abs(float(got) - float(want))
                print('modality', c, 'row', i, k, 'device', got, 'reference', want, 'diff %.3g' % d, 'bound %.3g' % bound)
                assert d <= bound, (c, i, k, got, want, bound)


def test_analyzer_matches_the_reference(dev, tmp_path, monkeypatch):
    from multitalent_amd import ops
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer
    z = np.load(G)
    folder = _golden_folder(z, str(tmp_path / 'cropped'))
    an = DatasetAnalyzer(folder, num_processes=2)
    assert an.patient_identifiers == list(z['names'])
    dp = an.analyze_dataset()
    class_dct, props = an.analyse_segmentations()
    assert list(dp.keys()) == list(z['dp_keys'])
    _check_against_golden(z, dp['intensityproperties'])
    assert dp['all_classes'] == [int(i) for i in z['all_classes']] and all(type(i) is int for i in dp['all_classes'])
    assert dp['modalities'] == dict(enumerate(str(m) for m in z['modalities']))
    assert type(dp['all_sizes'][0]).__name__ == str(z['all_sizes_type']) and np.array_equal(np.array(dp['all_sizes']), z['all_sizes'])
    assert np.array_equal(np.array(dp['all_spacings']), z['all_spacings'])
    assert list(dp['size_reductions'].keys()) == list(z['names'])
    assert np.array_equal(np.array(list(dp['size_reductions'].values())), z['size_reductions'])
    assert class_dct == json.loads(str(z['class_dct'])) and list(props.keys()) == list(z['names'])
    for n in z['names']:
        want = z[n + '/has_classes']
        assert list(props[n].keys()) == ['has_classes']
        assert props[n]['has_classes'].dtype == want.dtype and np.array_equal(props[n]['has_classes'], want)
    # the three files hold the returned objects
    for fname, obj in (('dataset_properties.pkl', dp), ('intensityproperties.pkl', dp['intensityproperties']), ('props_per_case.pkl', props)):
        with open(os.path.join(folder, fname), 'rb') as f:
            assert _same(pickle.load(f), obj), fname
    # two runs are bit-equal
    assert _same(DatasetAnalyzer(folder, num_processes=1).analyze_dataset(), dp)

    # overwrite=False reuses the files: the kernels are not reached
    def boom(*a, **k):
        raise AssertionError("the device path ran")
    monkeypatch.setattr(ops, 'fg_sample', boom)
    monkeypatch.setattr(ops, 'fg_sample_count', boom)
    monkeypatch.setattr(ops, 'label_presence', boom)
    lazy = DatasetAnalyzer(folder, overwrite=False)
    assert _same(lazy.analyze_dataset(), dp) and _same(lazy.analyse_segmentations()[1], props)
    with pytest.raises(AssertionError, match="device path ran"):
        DatasetAnalyzer(folder).collect_intensity_properties(2)


def test_compute_stats_and_nan_handling(dev, tmp_path):
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer
    z = np.load(G)
    empty = DatasetAnalyzer._compute_stats(np.zeros(0, dtype=np.float32))
    assert len(empty) == 7 and all(type(v) is float and np.isnan(v) for v in empty)
    v = np.round(np.random.RandomState(0).randn(2001) * 200).astype(np.float32)
    for arg in (v, torch.from_numpy(v), torch.from_numpy(v).to(dev), list(v)):
        got = DatasetAnalyzer._compute_stats(arg)
        want = (np.median(v), np.mean(v), np.std(v), np.min(v), np.max(v), np.percentile(v, 99.5), np.percentile(v, 0.5))
        assert all(type(g) is np.float32 for g in got)
        assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4] and got[5] == want[5] and got[6] == want[6]
        assert abs(got[1] - v.astype(np.float64).mean()) <= 1e-6 * 200 and abs(got[2] - v.astype(np.float64).std()) <= 1e-6 * 200
    v[77] = np.nan
    got = DatasetAnalyzer._compute_stats(v)
    assert len(got) == 7 and all(type(g) is np.float32 and np.isnan(g) for g in got)
    # a NaN among the sampled foreground voxels of one case: seven NaNs for the case and for the modality's global entry
    folder = _golden_folder(z, str(tmp_path / 'cropped'))
    name = str(z['names'][6])
    a = np.load(os.path.join(folder, name + '.npz'))['data']
    fg = np.flatnonzero(a[-1].reshape(-1) > 0)
    a[0].reshape(-1)[fg[10]] = np.nan                    # rank 10: sampled by the stride of 10
    a[1].reshape(-1)[fg[11]] = np.nan                    # rank 11: not sampled
    np.savez_compressed(os.path.join(folder, name + '.npz'), data=a)
    ip = DatasetAnalyzer(folder, num_processes=2).collect_intensity_properties(2)
    keys = list(z['stat_keys'])
    assert all(type(ip[0]['local_props'][name][k]) is np.float32 and np.isnan(ip[0]['local_props'][name][k]) for k in keys)
    assert all(type(ip[0][k]) is np.float32 and np.isnan(ip[0][k]) for k in keys)
    other = str(z['names'][5])
    assert all(np.isfinite(ip[0]['local_props'][other][k]) for k in keys)
    assert all(np.isfinite(ip[1]['local_props'][name][k]) and np.isfinite(ip[1][k]) for k in keys)
    assert ip[1]['mn'] == z['stats'][1, -1, 3] and ip[1]['percentile_99_5'] == pytest.approx(z['stats'][1, -1, 5], rel=1e-6)


# ---- chain: files -> offline cropper -> analyzer -> preprocessor ------------------------------------------------------------------------
def test_cropper_analyzer_preprocessor_chain(dev, tmp_path):
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer
    from multitalent_amd.preprocessing import cropping as host
    from multitalent_amd.preprocessing.device_cropping import ImageCropper, get_patient_identifiers_from_cropped_files
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    from multitalent_amd.utilities.nifti_io import write_image
    rs = np.random.RandomState(9)
    raw, out = tmp_path / 'raw', tmp_path / 'cropped'
    raw.mkdir()
    cases = []
    for i, shape in enumerate([(14, 20, 22), (12, 18, 25), (16, 16, 16)]):
        ct = np.round(rs.randn(*shape) * 150 + 30).astype(np.float32)
        mr = (rs.rand(*shape) * 900 + 5).astype(np.float32)
        seg = np.zeros(shape, dtype=np.float32)
        seg[3:9, 4:12, 5:13] = 1
        seg[5:7, 6:9, 7:10] = 2
        if i == 1:
            seg[9:11, 13:16, 15:20] = 3
        ct[:2], mr[:2] = 0, 0                                               # an all-zero border that the crop removes
        ct[:, :, :3], mr[:, :, :3] = 0, 0
        seg[:2] = 0
        seg[:, :, :3] = 0
        ct[2:5, 0:4, 3:7], mr[2:5, 0:4, 3:7] = 0, 0                         # zeros on a face of the box: outside the mask, label -1
        files = []
        for m, vol in enumerate((ct, mr)):
            files.append(str(raw / ('pat%d_%04d.nii.gz' % (i, m))))
            write_image(vol, files[-1], spacing=(0.8, 0.8, 2.5))
        files.append(str(raw / ('pat%d.nii.gz' % i)))
        write_image(seg, files[-1], spacing=(0.8, 0.8, 2.5))
        cases.append(files)
    cropper = ImageCropper(2, str(out))
    cropper.run_cropping(cases)
    names = ['pat0', 'pat1', 'pat2']
    assert get_patient_identifiers_from_cropped_files(str(out)) == names == cropper.get_patient_identifiers_from_cropped_files()
    assert sorted(os.listdir(out / 'gt_segmentations')) == ['pat%d.nii.gz' % i for i in range(3)]
    for files, name in zip(cases, names):
        with open(files[-1], 'rb') as a, open(out / 'gt_segmentations' / (name + '.nii.gz'), 'rb') as b:
            assert a.read() == b.read()
        data, seg, props = host.ImageCropper.crop_from_list_of_files(files[:-1], files[-1])
        got = np.load(out / (name + '.npz'))['data']
        want = np.vstack((data, seg))
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape and got.shape[1:] != tuple(props['original_size_of_raw_data'])
        assert got.tobytes() == want.tobytes()
        got_props = cropper.load_properties(name)
        assert list(got_props.keys()) == list(props.keys())
        for k in props:
            assert _same(got_props[k], props[k]) or (k == 'size_after_cropping' and tuple(got_props[k]) == tuple(props[k])), k
        assert got_props['classes'].dtype == np.float32 and list(got_props['classes']) == [-1, 0, 1, 2] + ([3] if name == 'pat1' else [])
    # a second call rewrites nothing; an incomplete case is redone; overwrite_existing rewrites
    stamp = {f: os.stat(out / f).st_mtime_ns for f in os.listdir(out) if f.endswith(('.npz', '.pkl'))}
    assert len(stamp) == 6
    cropper.run_cropping(cases, overwrite_existing=False)
    assert {f: os.stat(out / f).st_mtime_ns for f in stamp} == stamp
    os.remove(out / 'pat2.pkl')
    cropper.run_cropping(cases)
    assert os.path.isfile(out / 'pat2.pkl')
    assert all(os.stat(out / f).st_mtime_ns == stamp[f] for f in stamp if not f.startswith('pat2'))
    ImageCropper(1).run_cropping(cases[:1], overwrite_existing=True, output_folder=str(out))
    assert os.stat(out / 'pat0.npz').st_mtime_ns > stamp['pat0.npz'] and os.stat(out / 'pat1.npz').st_mtime_ns == stamp['pat1.npz']
    # the analyzer on the cropper's folder, against numpy
    with open(out / 'dataset.json', 'w') as f:
        json.dump({'modality': {'0': 'CT', '1': 'MR'}, 'labels': {'0': 'background', '1': 'a', '2': 'b', '3': 'c'}}, f)
    dp = DatasetAnalyzer(str(out), num_processes=2).analyze_dataset()
    arrays = [np.load(out / (n + '.npz'))['data'] for n in names]
    for c in (0, 1):
        v = np.concatenate([a[c][a[-1] > 0][::10] for a in arrays])
        s = np.sort(v).astype(np.float64)
        ip = dp['intensityproperties'][c]
        assert ip['mn'] == v.min() and ip['mx'] == v.max()
        for k, q, want in (('median', 50.0, np.median(v)), ('percentile_99_5', 99.5, np.percentile(v, 99.5)),
                           ('percentile_00_5', 0.5, np.percentile(v, 0.5))):
            vi = (len(s) - 1) * q / 100
            lo = int(np.floor(vi))
            dev64 = abs(float(want) - (s[lo] + (s[min(lo + 1, len(s) - 1)] - s[lo]) * (vi - lo)))
            assert abs(float(ip[k]) - float(want)) <= 2 * dev64 + float(np.spacing(np.abs(np.float32(want)))), (c, k, ip[k], want)
        for k, want in (('mean', s.mean()), ('sd', s.std())):
            dev64 = abs(float(getattr(np, 'std' if k == 'sd' else k)(v)) - want)
            assert abs(float(ip[k]) - want) <= 2 * dev64 + 1e-6 * max(1.0, abs(want)), (c, k, ip[k], want)
    assert dp['all_classes'] == [1, 2, 3] and [tuple(s) for s in dp['all_sizes']] == [a.shape[1:] for a in arrays]
    # the next stage accepts the folder and the fingerprint
    pre = GenericPreprocessor({0: 'CT', 1: 'nonCT'}, {0: False, 1: False}, [0, 1, 2], dp['intensityproperties'])
    pre.run([np.array([2.5, 0.8, 0.8])], str(out), str(tmp_path / 'pre'), 'nnUNetData_plans', num_threads=2)
    stage = tmp_path / 'pre' / 'nnUNetData_plans_stage0'
    assert sorted(os.listdir(stage)) == sorted([n + e for n in names for e in ('.npz', '.pkl')])
    for n, a in zip(names, arrays):
        b = np.load(stage / (n + '.npz'))['data']
        ip = dp['intensityproperties'][0]
        want = (np.clip(a[0], ip['percentile_00_5'], ip['percentile_99_5']) - ip['mean']) / ip['sd']
        assert b.shape == a.shape and np.array_equal(b[-1], a[-1]) and np.abs(b[0] - want).max() <= 2e-4
