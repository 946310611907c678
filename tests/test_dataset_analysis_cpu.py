"""Host side of the dataset fingerprint (multitalent_amd/experiment_planning/DatasetAnalyzer.py) and of the offline cropper against the
REAL reference's DatasetAnalyzer (tools/oracle_gen/make_golden_dataset_analysis.py -> golden/dataset_analysis.npz) and numpy.
Bound of an interpolated value: 2 x dev64 + 1 float32 ulp of the value, dev64 = |numpy's float32 result - the same formula in
float64 on the sorted samples| (recorded per value in the golden, computed here for the random arrays): the host interpolates from
exact neighbours in one rounding order, numpy may use another."""
import inspect
import json
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataset_analysis.npz')
INTERP = (('median', 'median'), ('percentile_99_5', 99.5), ('percentile_00_5', 0.5))


def _formula64(s, q):
    n = len(s)
    if q == 'median':
        return (s[(n - 1) // 2] + s[n // 2]) / 2
    vi = (n - 1) * (q / 100.0)
    lo = int(np.floor(vi))
    return s[lo] + (s[min(lo + 1, n - 1)] - s[lo]) * (vi - lo)


def _bound(dev64, value):
    return 2 * float(dev64) + float(np.spacing(np.abs(np.float32(value))))


def test_interpolate_reproduces_the_golden_from_its_neighbours():
    from multitalent_amd.experiment_planning.DatasetAnalyzer import _interpolate
    z = np.load(G)
    keys = list(z['stat_keys'])
    checked = 0
    for c in range(z['stats'].shape[0]):
        for i, n in enumerate(z['nsamples']):
            if n == 0:
                continue
            for j, (k, q) in enumerate(INTERP):
                lo, hi = z['neighbours'][c, i, j]
                got, want = _interpolate(lo, hi, int(n), q), z['stats'][c, i, keys.index(k)]
                assert type(got) is np.float32
                d, b = abs(float(got) - float(want)), _bound(z['dev64'][c, i, keys.index(k)], want)
                print(c, i, k, 'n', int(n), 'got', got, 'want', want, 'diff', d, 'bound', b)
                assert d <= b
                checked += 1
    assert checked == 2 * 7 * 3                       # six cases with samples and the global entry, two modalities


@pytest.mark.parametrize("n", [1, 2, 3, 7, 200, 201, 100003])
def test_interpolate_against_numpy(n):
    from multitalent_amd.experiment_planning.DatasetAnalyzer import _interpolate, _neighbour_ranks, _stat_ranks
    rs = np.random.RandomState(n)
    for values in ((rs.randn(n) * 175 + 63).astype(np.float32), np.clip(np.round(rs.randn(n) * 300), -1024, 3071).astype(np.float32)):
        s32 = np.sort(values)
        s64 = s32.astype(np.float64)
        for q, want in (('median', np.median(values)), (99.5, np.percentile(values, 99.5)), (0.5, np.percentile(values, 0.5))):
            lo, hi = _neighbour_ranks(n, q)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1
            got = _interpolate(s32[lo], s32[hi], n, q)
            dev64 = abs(float(want) - _formula64(s64, q))
            print('n', n, q, 'got', got, 'numpy', want, 'diff', abs(float(got) - float(want)), 'bound', _bound(dev64, want))
            assert type(got) is np.float32 and abs(float(got) - float(want)) <= _bound(dev64, want)
    ranks = _stat_ranks(n)
    assert len(ranks) == 8 and ranks[0] == 0 and ranks[1] == n - 1 and all(0 <= r < n for r in ranks)


def test_signatures_are_the_references():
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer
    from multitalent_amd.preprocessing.device_cropping import ImageCropper
    z = np.load(G)
    sigs = [k for k in z.files if k.startswith('sig/')]
    assert len(sigs) == 10
    for k in sigs:
        assert list(inspect.signature(getattr(DatasetAnalyzer, k[4:])).parameters) == list(z[k]), k
    assert isinstance(inspect.getattr_static(DatasetAnalyzer, '_compute_stats'), staticmethod)
    assert list(inspect.signature(ImageCropper.__init__).parameters) == ['self', 'num_threads', 'output_folder']
    assert list(inspect.signature(ImageCropper.run_cropping).parameters) == ['self', 'list_of_files', 'overwrite_existing', 'output_folder']
    assert list(inspect.signature(ImageCropper.load_crop_save).parameters) == ['self', 'case', 'case_identifier', 'overwrite_existing']
    for name in ('get_list_of_cropped_files', 'get_patient_identifiers_from_cropped_files', 'load_properties', 'save_properties'):
        assert callable(getattr(ImageCropper, name))
    assert isinstance(inspect.getattr_static(ImageCropper, 'crop'), staticmethod)
    assert isinstance(inspect.getattr_static(ImageCropper, 'crop_from_list_of_files'), staticmethod)


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


def test_key_order_and_types_of_a_patched_run(tmp_path, monkeypatch):
    """The device statistics replaced by numpy on the same samples: keys, their order, the value types and the files are the
    reference's, and the host combination meets the golden within the bounds."""
    import torch
    from multitalent_amd.experiment_planning import DatasetAnalyzer as da
    z = np.load(G)
    folder = _golden_folder(z, str(tmp_path / 'cropped'))

    def fake_statistics(self, M):
        local, glob, nans = [[] for _ in range(M)], [], []
        per_mod = [[] for _ in range(M)]
        for p in self.patient_identifiers:
            a = self._load_case(p)
            nans.append([0] * M)
            for c in range(M):
                v = a[c][a[-1] > 0][::10]
                per_mod[c].append(v)
                local[c].append(self._numpy_pending(v))
        for c in range(M):
            glob.append(self._numpy_pending(np.concatenate(per_mod[c])))
        return local, glob, np.array(nans)

    def numpy_pending(v):
        n = len(v)
        if n == 0:
            return da._Pending(0)
        s = np.sort(v)
        return da._Pending(n, s[da._stat_ranks(n)], np.array([n, v.astype(np.float64).mean(), v.astype(np.float64).std()]))

    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(da.DatasetAnalyzer, '_device_statistics', fake_statistics)
    monkeypatch.setattr(da.DatasetAnalyzer, '_numpy_pending', staticmethod(numpy_pending), raising=False)
    an = da.DatasetAnalyzer(folder, num_processes=2)
    assert an.patient_identifiers == list(z['names'])
    dp = an.analyze_dataset()
    assert list(dp.keys()) == list(z['dp_keys'])
    ip = dp['intensityproperties']
    assert type(ip) is OrderedDict and list(ip.keys()) == [0, 1]
    keys = list(z['stat_keys'])
    for c in (0, 1):
        assert type(ip[c]) is OrderedDict and list(ip[c].keys()) == list(z['ip_keys'])
        assert type(ip[c]['local_props']) is OrderedDict and list(ip[c]['local_props'].keys()) == list(z['names'])
        rows = [ip[c]['local_props'][n] for n in z['names']] + [ip[c]]
        for i, row in enumerate(rows):
            if i < len(z['names']):
                assert type(row) is OrderedDict and list(row.keys()) == keys
            for j, k in enumerate(keys):
                assert type(row[k]).__name__ == str(z['types'][c, i, j]), (c, i, k, type(row[k]))
                want = z['stats'][c, i, j]
                if np.isnan(want):
                    assert np.isnan(row[k])
                elif k in ('mn', 'mx'):
                    assert row[k] == want
                else:
                    b = _bound(z['dev64'][c, i, j], want) if k not in ('mean', 'sd') else 2 * z['dev64'][c, i, j] + 1e-6 * max(1.0, abs(want))
                    assert abs(float(row[k]) - float(want)) <= b, (c, i, k, row[k], want, b)
    assert dp['all_classes'] == [int(i) for i in z['all_classes']] and dp['modalities'] == dict(enumerate(str(m) for m in z['modalities']))
    assert type(dp['all_sizes'][0]).__name__ == str(z['all_sizes_type']) and np.array_equal(np.array(dp['all_sizes']), z['all_sizes'])
    assert np.array_equal(np.array(dp['all_spacings']), z['all_spacings'])
    assert list(dp['size_reductions'].keys()) == list(z['names'])
    assert np.array_equal(np.array(list(dp['size_reductions'].values())), z['size_reductions'])
    assert an.get_classes() == json.loads(str(z['class_dct']))
    for fname in ('dataset_properties.pkl', 'intensityproperties.pkl'):
        assert os.path.isfile(os.path.join(folder, fname))
    with open(os.path.join(folder, 'intensityproperties.pkl'), 'rb') as f:
        back = pickle.load(f)
    assert list(back[1].keys()) == list(z['ip_keys']) and back[1]['mn'] == ip[1]['mn']


def test_no_device_fails_loudly(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    from multitalent_amd.experiment_planning.DatasetAnalyzer import DatasetAnalyzer
    from multitalent_amd.preprocessing.device_cropping import ImageCropper
    z = np.load(G)
    an = DatasetAnalyzer(_golden_folder(z, str(tmp_path / 'cropped')))
    with pytest.raises(RuntimeError, match="HIP device only"):
        an.collect_intensity_properties(2)
    with pytest.raises(RuntimeError, match="HIP device only"):
        an.analyse_segmentations()
    with pytest.raises(RuntimeError, match="HIP device only"):
        DatasetAnalyzer._compute_stats(np.zeros(3, dtype=np.float32))
    assert not os.path.exists(an.intensityproperties_file) and not os.path.exists(an.props_per_case_file)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ImageCropper(2, str(tmp_path / 'out')).run_cropping([[str(tmp_path / 'a_0000.nii.gz'), None]])
    assert os.path.isdir(tmp_path / 'out') and os.listdir(tmp_path / 'out') == []


def test_patient_identifiers_from_cropped_files(tmp_path):
    from multitalent_amd.preprocessing import device_cropping as dc
    for name in ('b_002.npz', 'a_010.npz', 'a_001.npz', 'a_001.pkl', 'dataset.json', 'notes.npz.txt'):
        (tmp_path / name).write_bytes(b'')
    (tmp_path / 'gt_segmentations.npz').mkdir()                      # a directory is no file
    assert dc.get_patient_identifiers_from_cropped_files(str(tmp_path)) == ['a_001', 'a_010', 'b_002']
    cropper = dc.ImageCropper(1, str(tmp_path))
    assert cropper.get_patient_identifiers_from_cropped_files() == ['a_001', 'a_010', 'b_002']
    assert cropper.get_list_of_cropped_files() == [str(tmp_path / (n + '.npz')) for n in ('a_001', 'a_010', 'b_002')]
    cropper.save_properties('a_010', {'x': 1})
    assert cropper.load_properties('a_010') == {'x': 1}
