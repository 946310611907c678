"""Golden vectors for the dataset fingerprint on the device: the REAL reference's DatasetAnalyzer
(experiment_planning/DatasetAnalyzer.py) on a small synthetic folder of cropped cases.  The few batchgenerators file helpers the
reference module needs (third party, absent here) are added below: subfiles, load_json, save_pickle, load_pickle.
Writes tests/golden/dataset_analysis.npz: the cases, every number analyze_dataset() and analyse_segmentations() return, the order
statistics each interpolated value is formed from, and per value `dev64`: the absolute difference between the reference's float32
result and the same formula in float64 on the sorted samples (float64 moments for mean and sd).
Run: python tools/oracle_gen/make_golden_dataset_analysis.py"""
import inspect, io, json, os, pickle, sys, tempfile, zipfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import
ref_import.install()
import batchgenerators.utilities.file_and_folder_operations as ffo


def subfiles(folder, join=True, prefix=None, suffix=None, sort=True):
    """Restatement of batchgenerators' subfiles: the files of a folder, filtered by prefix / suffix, sorted."""
    res = [os.path.join(folder, i) if join else i for i in os.listdir(folder)
           if os.path.isfile(os.path.join(folder, i)) and (prefix is None or i.startswith(prefix)) and (suffix is None or i.endswith(suffix))]
    if sort:
        res.sort()
    return res


def load_json(file):
    with open(file, 'r') as f:
        return json.load(f)


def save_pickle(obj, file, mode='wb'):
    with open(file, mode) as f:
        pickle.dump(obj, f)


def load_pickle(file, mode='rb'):
    with open(file, mode) as f:
        return pickle.load(f)


for _f in (subfiles, load_json, save_pickle, load_pickle):
    setattr(ffo, _f.__name__, _f)
ffo.__all__ = sorted(set(ffo.__all__) | {'subfiles', 'load_json', 'save_pickle', 'load_pickle'})
import nnunet.experiment_planning.DatasetAnalyzer as ref_da

STAT_KEYS = ('median', 'mean', 'sd', 'mn', 'mx', 'percentile_99_5', 'percentile_00_5')
INTERP = {'median': 'median', 'percentile_99_5': 99.5, 'percentile_00_5': 0.5}
DATASET_JSON = {"name": "golden", "modality": {"0": "CT", "1": "MR"},
                "labels": {"0": "background", "1": "organ", "2": "lesion", "3": "vessel"}}
METHODS = ('__init__', 'load_properties_of_cropped', 'get_classes', 'get_modalities', 'get_sizes_and_spacings_after_cropping',
           'get_size_reduction_by_cropping', 'analyse_segmentations', 'collect_intensity_properties', 'analyze_dataset', '_compute_stats')


def make_case(rs, shape, kind):
    """Two modalities (integer-valued HU with many ties, and a real-valued one) and a label map -1..3 in blocks."""
    hu = np.clip(np.round(rs.randn(*shape) * 180 + 40), -1024, 3071).astype(np.float32)
    hu[rs.rand(*shape) < 0.3] = -1000.0                                   # air: a heavy tie, negative
    mr = (rs.randn(*shape) * 175 + 63).astype(np.float32)
    seg = np.zeros(shape, dtype=np.float32)
    seg[:, :2, :] = -1
    seg[:, :, shape[2] - 3:] = -1
    if kind == 'empty':
        pass
    elif kind == 'one':
        seg[3, 7, 5] = 2
    elif kind == 'seven':
        seg[4, 6, 3:10] = 1
    elif kind == 'mult10':                                                # 5*4*6 + 2*5*3 = 150
        seg[2:7, 4:8, 2:8] = 1
        seg[9:11, 10:15, 10:13] = 3
    elif kind == 'one_mod10':                                             # 6*10*10 + 1 = 601
        seg[5:11, 8:18, 6:16] = 2
        seg[1, 3, 1] = 3
    elif kind == 'constant':
        seg[3:12, 5:16, 4:20] = 1
        seg[13:16, 3:9, 2:9] = 2
        seg[6:8, 18:21, 3:8] = 3
        mr[seg > 0] = 37.5
    else:                                                                 # ordinary: labels 1 and 2, no 3
        seg[2:15, 4:20, 3:18] = 1
        seg[6:12, 8:14, 6:12] = 2
        seg[16:18, 5:9, 10:20] = 2
    return np.stack((hu, mr)), seg[None]


CASES = [('case_000_empty', (18, 22, 26), 'empty'), ('case_001_one', (16, 24, 20), 'one'), ('case_002_seven', (17, 20, 28), 'seven'),
         ('case_003_mult10', (20, 24, 28), 'mult10'), ('case_004_one_mod10', (19, 23, 27), 'one_mod10'),
         ('case_005_constant', (20, 24, 28), 'constant'), ('case_006_ordinary', (20, 24, 28), 'ordinary')]


def neighbour_ranks(n, q):
    """The ranks numpy combines: the two middle elements for the median; floor of the float32 virtual index (n - 1) * (q / float32(100))
    and its successor for a percentile (numpy forms the quantile and the index in the sample's own type)."""
    if q == 'median':
        return (n - 1) // 2, n // 2
    vi = np.float32((n - 1) * np.true_divide(q, np.float32(100)))
    if not vi < n - 1:
        return n - 1, n - 1
    lo = int(np.floor(vi))
    return lo, min(lo + 1, n - 1)


def formula64(s, q):
    n = len(s)
    if q == 'median':
        return (s[(n - 1) // 2] + s[n // 2]) / 2
    vi = (n - 1) * (q / 100.0)
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    return s[lo] + (s[hi] - s[lo]) * (vi - lo)


def describe(values, samples):
    """values: the reference's seven results for `samples` -> (stats, dev64, neighbours, type names)."""
    stats = np.array([np.float32(v) for v in values], dtype=np.float32)
    types = [type(v).__name__ for v in values]
    dev = np.zeros(7)
    neigh = np.full((3, 2), np.nan, dtype=np.float32)
    n = len(samples)
    if n:
        s = np.sort(np.asarray(samples, dtype=np.float32)).astype(np.float64)
        want = {'mean': s.mean(), 'sd': s.std(), 'mn': s[0], 'mx': s[-1]}
        want.update({k: formula64(s, q) for k, q in INTERP.items()})
        for i, k in enumerate(STAT_KEYS):
            dev[i] = abs(float(values[i]) - want[k])
        assert dev[3] == 0 and dev[4] == 0
        for j, (k, q) in enumerate(INTERP.items()):
            lo, hi = neighbour_ranks(n, q)
            neigh[j] = (s[lo], s[hi])
    return stats, dev, neigh, types


def main():
    rs = np.random.RandomState(2024)
    rec = {}
    with tempfile.TemporaryDirectory() as folder:
        with open(os.path.join(folder, 'dataset.json'), 'w') as f:
            json.dump(DATASET_JSON, f)
        samples = {}
        for i, (name, shape, kind) in enumerate(CASES):
            data, seg = make_case(rs, shape, kind)
            raw = np.array(shape) + np.array([i % 3, 2 * (i % 2), 5])
            props = {'original_size_of_raw_data': raw, 'original_spacing': np.array([2.5 - 0.25 * i, 0.8 + 0.01 * i, 0.8 + 0.01 * i]),
                     'size_after_cropping': tuple(int(j) for j in shape), 'crop_bbox': [[0, int(j)] for j in shape]}
            np.savez_compressed(os.path.join(folder, name + '.npz'), data=np.vstack((data, seg)))
            save_pickle(props, os.path.join(folder, name + '.pkl'))
            rec[name + '/data'] = data
            rec[name + '/seg'] = seg.astype(np.int8)
            rec[name + '/raw_size'] = raw
            rec[name + '/spacing'] = props['original_spacing']
            samples[name] = [data[c][seg[0] > 0][::10] for c in range(2)]
            print(name, shape, 'foreground', int((seg > 0).sum()), 'samples', len(samples[name][0]))
        an = ref_da.DatasetAnalyzer(folder, num_processes=2)
        dp = an.analyze_dataset()
        class_dct, props_per_case = an.analyse_segmentations()
        for fname in ('dataset_properties.pkl', 'intensityproperties.pkl', 'props_per_case.pkl'):
            assert os.path.isfile(os.path.join(folder, fname)), fname
    names = [c[0] for c in CASES]
    assert list(props_per_case.keys()) == names and an.patient_identifiers == names
    ip = dp['intensityproperties']
    assert list(ip.keys()) == [0, 1]
    stats = np.zeros((2, len(names) + 1, 7), dtype=np.float32)
    dev = np.zeros((2, len(names) + 1, 7))
    neigh = np.zeros((2, len(names) + 1, 3, 2), dtype=np.float32)
    types = np.zeros((2, len(names) + 1, 7), dtype='U16')
    nsamp = np.array([len(samples[n][0]) for n in names] + [sum(len(samples[n][0]) for n in names)])
    for c in (0, 1):
        assert list(ip[c].keys()) == ['local_props'] + list(STAT_KEYS) and list(ip[c]['local_props'].keys()) == names
        for i, n in enumerate(names):
            assert list(ip[c]['local_props'][n].keys()) == list(STAT_KEYS)
            stats[c, i], dev[c, i], neigh[c, i], types[c, i] = describe([ip[c]['local_props'][n][k] for k in STAT_KEYS], samples[n][c])
        allv = np.concatenate([samples[n][c] for n in names])
        stats[c, -1], dev[c, -1], neigh[c, -1], types[c, -1] = describe([ip[c][k] for k in STAT_KEYS], allv)
    # the restated ranks and numpy's float32 interpolation reproduce the reference bit for bit from the recorded neighbours
    for c in (0, 1):
        for i in range(len(names) + 1):
            n = int(nsamp[i])
            for j, (k, q) in enumerate(INTERP.items()):
                if n == 0:
                    continue
                a, b = neigh[c, i, j]
                if q == 'median':
                    got = a if n % 2 else np.float32(np.float32(a + b) / np.float32(2))
                else:
                    vi = np.float32((n - 1) * np.true_divide(q, np.float32(100)))
                    t = np.float32(vi - np.floor(vi)) if vi < n - 1 else np.float32(0)
                    d = np.float32(b - a)
                    got = np.float32(b - d * np.float32(1 - t)) if t >= 0.5 else np.float32(a + d * t)
                assert got == stats[c, i, STAT_KEYS.index(k)], (c, i, k, got, stats[c, i, STAT_KEYS.index(k)])
    assert np.isnan(stats[:, 0]).all() and (types[:, 0] == 'float').all() and (types[:, 1:] == 'float32').all()
    assert nsamp[1] == 1 and nsamp[2] == 1 and stats[1, 5, 2] == 0
    print('largest dev64 in float32 ulps of the value:',
          float(np.nanmax(dev[:, 1:, [0, 5, 6]] / np.maximum(np.spacing(np.abs(stats[:, 1:, [0, 5, 6]])), 1e-45))))
    rec['names'] = np.array(names)
    rec['dataset_json'] = np.array(json.dumps(DATASET_JSON))
    rec['stat_keys'] = np.array(STAT_KEYS)
    rec['stats'], rec['dev64'], rec['neighbours'], rec['types'], rec['nsamples'] = stats, dev, neigh, types, nsamp
    rec['dp_keys'] = np.array(list(dp.keys()))
    rec['ip_keys'] = np.array(list(ip[0].keys()))
    rec['all_sizes'] = np.array(dp['all_sizes'])
    rec['all_sizes_type'] = np.array(type(dp['all_sizes'][0]).__name__)
    rec['all_spacings'] = np.array(dp['all_spacings'])
    rec['all_classes'] = np.array(dp['all_classes'])
    rec['modalities'] = np.array([dp['modalities'][k] for k in sorted(dp['modalities'])])
    assert list(dp['size_reductions'].keys()) == names
    rec['size_reductions'] = np.array([dp['size_reductions'][n] for n in names])
    rec['class_dct'] = np.array(json.dumps(class_dct))
    for n in names:
        assert list(props_per_case[n].keys()) == ['has_classes']
        rec[n + '/has_classes'] = props_per_case[n]['has_classes']
    for m in METHODS:
        rec['sig/' + m] = np.array(list(inspect.signature(getattr(ref_da.DatasetAnalyzer, m)).parameters))
    dst = os.path.normpath(os.path.join(HERE, '..', '..', 'tests', 'golden', 'dataset_analysis.npz'))
    with zipfile.ZipFile(dst, 'w', zipfile.ZIP_DEFLATED) as z:           # fixed member dates: the file is reproducible byte for byte
        for k in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print('wrote', dst, os.path.getsize(dst) // 1024, 'KiB')


if __name__ == '__main__':
    main()
