"""Connected-component postprocessing on the device: the labelling (mt_cc_label3d) against scipy.ndimage.label, the removal
against the REAL reference's outputs (tests/golden/postprocessing.* from tools/oracle_gen/make_golden_postprocessing.py),
`determine_postprocessing` against the reference's decisions, and the search at the end of `nnUNetTrainer.validate`."""
import ast
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def golden():
    return np.load(os.path.join(HERE, 'golden', 'postprocessing.npz')), json.load(open(os.path.join(HERE, 'golden', 'postprocessing.json')))


def expected_labels(mask):
    """scipy's partition -> (labels = smallest linear index of the component or -1, sizes at that index, count, largest)"""
    lmap, n = ndimage.label(mask)
    lab = np.full(mask.shape, -1, np.int64).ravel()
    sizes = np.zeros(mask.size, np.int64)
    if n:
        flat = lmap.ravel()
        idx = np.flatnonzero(flat)
        first = np.full(n + 1, np.iinfo(np.int64).max)
        np.minimum.at(first, flat[idx], idx)
        lab[idx] = first[flat[idx]]
        cnt = np.bincount(flat, minlength=n + 1)
        sizes[first[1:]] = cnt[1:]
    return lab.reshape(mask.shape), sizes.reshape(mask.shape), n, int(sizes.max()) if n else 0


def run_label(seg, member):
    from multitalent_amd import ops
    out = []
    for _ in range(2):
        labels, sizes, stats = ops.cc_label3d(seg, member)
        torch.cuda.synchronize()
        out.append((labels.cpu().numpy(), sizes.cpu().numpy(), stats.cpu().numpy()))
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1])), "two runs differ"
    return out[0]


def check_label(vol, member=None):
    vol = np.ascontiguousarray(vol, dtype=np.uint8)
    if member is None:
        member = np.zeros(256, bool)
        member[1:] = True
    mask = member[vol]
    lab, sz, st = run_label(torch.from_numpy(vol).cuda(), member)
    elab, esz, n, mx = expected_labels(mask)
    assert np.array_equal(lab, elab), "labels differ from scipy's partition at %d voxels" % int((lab != elab).sum())
    assert np.array_equal(sz, esz)
    assert int(st[0]) == n and int(st[1]) == mx
    return n


def serpentine(D, H, W):
    """a one-voxel-wide path through every brick: rows along W on even h of even d, joined at alternating ends, slices
    joined at alternating corners; the smallest index (0, 0, 0) is one end of a path of ~D*H*W/4 voxels."""
    v = np.zeros((D, H, W), np.uint8)
    end = (0, 0)
    for d in range(0, D, 2):
        hs = list(range(0, H, 2)) if (d // 2) % 2 == 0 else list(range(0, H, 2))[::-1]
        for j, h in enumerate(hs):
            v[d, h, :] = 1
            if j + 1 < len(hs):
                w = W - 1 if j % 2 == 0 else 0
                v[d, min(h, hs[j + 1]) + 1, w] = 1
        end = (hs[-1], W - 1 if (len(hs) - 1) % 2 == 0 else 0)
        if d + 2 < D:
            v[d + 1, end[0], end[1]] = 1
    return v


@pytest.mark.parametrize('case', ['empty', 'full', 'single', 'checker', '1x1xN', 'Nx1x1', '1xNxM', 'odd', 'serpentine', 'multilabel'])
def test_labelling_matches_scipy(case):
    rng = np.random.default_rng(3)
    if case == 'empty':
        vol = np.zeros((9, 17, 33), np.uint8)
    elif case == 'full':
        vol = np.ones((9, 17, 33), np.uint8)
    elif case == 'single':
        vol = np.zeros((19, 23, 37), np.uint8); vol[11, 17, 29] = 1
    elif case == 'checker':
        z, y, x = np.indices((10, 21, 34))
        vol = ((z + y + x) % 2).astype(np.uint8)
    elif case == '1x1xN':
        vol = (rng.random((1, 1, 1000)) < 0.7).astype(np.uint8)
    elif case == 'Nx1x1':
        vol = (rng.random((1000, 1, 1)) < 0.7).astype(np.uint8)
    elif case == '1xNxM':
        vol = (rng.random((1, 131, 257)) < 0.55).astype(np.uint8)
    elif case == 'odd':
        vol = (rng.random((67, 131, 257)) < 0.3116).astype(np.uint8)
    elif case == 'serpentine':
        vol = serpentine(21, 45, 53)
        assert vol[0, 0, 0] == 1
    else:
        vol = rng.integers(0, 6, (40, 48, 56)).astype(np.uint8)
        member = np.zeros(256, bool); member[[2, 5]] = True
        n = check_label(vol, member)
        assert n > 1
        return
    n = check_label(vol)
    if case == 'serpentine':
        assert n == 1
    if case == 'checker':
        assert n == int(vol.sum())


@pytest.mark.parametrize('density', [0.05, 0.25, 0.3116, 0.5, 0.9])
def test_labelling_random_densities(density):
    rng = np.random.default_rng(int(density * 1e4))
    check_label((rng.random((48, 80, 96)) < density).astype(np.uint8))


def test_labelling_percolation_400():
    rng = np.random.default_rng(400)
    check_label((rng.random((400, 400, 400)) < 0.3116).astype(np.uint8))


def _fixture_dicts(entry):
    f = lambda lst: {ast.literal_eval(k): v for k, v in lst}
    return f(entry['largest_removed']), f(entry['kept_size'])


@pytest.mark.parametrize('as_tensor', [False, True])
def test_remove_matches_reference(as_tensor):
    from multitalent_amd.postprocessing.connected_components import remove_all_but_the_largest_connected_component
    z, meta = golden()
    for e in meta['a']:
        img = z['a/%s/in' % e['name']].copy()
        fwc = ast.literal_eval(e['for_which_classes'])
        mins = ast.literal_eval(e['min_sizes'])
        arg = torch.from_numpy(img).cuda() if as_tensor else img
        out, lr, ks = remove_all_but_the_largest_connected_component(arg, fwc, e['volume_per_voxel'], mins)
        if as_tensor:
            assert torch.is_tensor(out) and out.is_cuda and out.data_ptr() == arg.data_ptr()
            out = out.cpu().numpy()
        else:
            assert out is img                                              # modified in place
        assert np.array_equal(out, z['a/%s/out' % e['name']]), e['name']
        elr, eks = _fixture_dicts(e)
        assert list(lr) == list(elr) and list(ks) == list(eks), e['name']
        for k in elr:
            assert lr[k] == elr[k] and ks[k] == eks[k], (e['name'], k)              # exact fp64
            assert (lr[k] is None) or type(lr[k]) is float


def test_input_checks_before_any_launch():
    from multitalent_amd.postprocessing.connected_components import remove_all_but_the_largest_connected_component as rm
    with pytest.raises(ValueError, match="3-D"):
        rm(np.zeros((4, 5), np.uint8), [1], 1.0)
    with pytest.raises(ValueError, match="3-D"):
        rm(torch.zeros((2, 4, 5, 6), dtype=torch.uint8, device='cuda'), [1], 1.0)
    big = np.zeros((6, 7, 8), np.int16); big[1, 1, 1] = 300
    with pytest.raises(ValueError, match="0..255"):
        rm(big, [1], 1.0)
    with pytest.raises(ValueError, match="0..255"):
        rm(torch.from_numpy(big).cuda(), [1], 1.0)
    huge = np.broadcast_to(np.zeros(1, np.uint8), (2048, 2048, 1024))      # 2^32 voxels, nothing allocated
    with pytest.raises(ValueError, match="int32"):
        rm(huge, [1], 1.0)
    with pytest.raises(RuntimeError, match="HIP device only"):
        rm(torch.zeros((4, 5, 6), dtype=torch.uint8), [1], 1.0)


def test_load_remove_save_keeps_geometry(tmp_path):
    from multitalent_amd.postprocessing.connected_components import load_remove_save
    from multitalent_amd.utilities.nifti_io import read_image, write_image
    z, meta = golden()
    img = z['a/none/in']
    spacing, origin = (0.7, 0.8, 2.5), (10.0, -20.5, 3.25)
    c, s = np.cos(0.3), np.sin(0.3)
    direction = (c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0)
    write_image(img, str(tmp_path / 'in.nii.gz'), spacing, origin, direction)
    lr, ks = load_remove_save(str(tmp_path / 'in.nii.gz'), str(tmp_path / 'out.nii.gz'), [1, 2, 3])
    back_in = read_image(str(tmp_path / 'in.nii.gz'))
    out = read_image(str(tmp_path / 'out.nii.gz'))
    assert np.allclose(out.spacing, back_in.spacing, rtol=0, atol=1e-6) and np.allclose(out.origin, back_in.origin, rtol=0, atol=1e-5)
    assert np.allclose(out.direction, back_in.direction, rtol=0, atol=1e-6)
    vpv = float(np.prod(back_in.spacing, dtype=np.float64))
    kept = {k: int(v) for k, v in [(1, 2668), (2, 1867), (3, 417)]}                 # voxel counts of the reference's 'none' case
    for k in (1, 2, 3):
        assert ks[k] == float(np.float64(kept[k]) * np.float64(vpv))
    assert np.array_equal(np.asarray(out.array), z['a/none/out'])


def _strip_np(s):
    return re.sub(r'np\.float64\(([^)]*)\)', r'\1', s)


@pytest.mark.parametrize('scenario', ['fg_accepted', 'fg_rejected_per_class', 'single_class', 'advanced'])
def test_determine_postprocessing_matches_reference(tmp_path, scenario):
    from multitalent_amd.evaluation.evaluator import aggregate_scores
    from multitalent_amd.postprocessing.connected_components import determine_postprocessing
    from multitalent_amd.utilities.nifti_io import read_image, write_image
    z, meta = golden()
    sc = [s for s in meta['b'] if s['name'] == scenario][0]
    base = tmp_path / 'fold'
    for c in sc['cases']:
        sp = tuple(float(i) for i in z['b/%s/%s/spacing' % (scenario, c)])
        for sub, what in (('validation_raw', 'raw'), ('gt_segmentations', 'gt')):
            (base / sub).mkdir(parents=True, exist_ok=True)
            write_image(z['b/%s/%s/%s' % (scenario, c, what)], str(base / sub / (c + '.nii.gz')), sp, (1.5, -2.0, 3.0))
    aggregate_scores([[str(base / 'validation_raw' / (c + '.nii.gz')), str(base / 'gt_segmentations' / (c + '.nii.gz'))] for c in sc['cases']],
                     labels=sc['labels'], json_output_file=str(base / 'validation_raw' / 'summary.json'))
    determine_postprocessing(str(base), str(base / 'gt_segmentations'), 'validation_raw', final_subf_name='validation_final',
                             advanced_postprocessing=sc['advanced'])
    got = json.load(open(str(base / 'postprocessing.json')))
    ref = sc['postprocessing']
    assert sorted(got) == sorted(ref)
    assert got['for_which_classes'] == ref['for_which_classes']
    assert ast.literal_eval(got['min_valid_object_sizes']) == ast.literal_eval(_strip_np(ref['min_valid_object_sizes']))
    for k in ('num_samples', 'validation_raw', 'validation_final'):
        assert got[k] == ref[k]
    for k in ('dc_per_class_raw', 'dc_per_class_pp_all', 'dc_per_class_pp_per_class'):
        assert sorted(got[k]) == sorted(ref[k])
        for c in ref[k]:
            assert abs(got[k][c] - ref[k][c]) <= 1e-12, (k, c)
    for c in sc['cases']:
        assert np.array_equal(np.asarray(read_image(str(base / 'validation_final' / (c + '.nii.gz'))).array),
                              z['b/%s/%s/final' % (scenario, c)]), c
    assert os.path.isfile(str(base / 'validation_final' / 'summary.json'))
    assert sorted(os.listdir(str(base))) == sc['folders']                 # temp_allClasses / temp_perClass are gone


# ---- the search at the end of nnUNetTrainer.validate --------------------------------------------------------------------------


def host_remove(img, classes):
    """the reference's removal restated with scipy (no minimum sizes)"""
    img = img.copy()
    for c in classes:
        members = tuple(c) if isinstance(c, (list, tuple)) else (c,)
        mask = np.isin(img, members)
        lmap, n = ndimage.label(mask)
        if n == 0:
            continue
        cnt = np.bincount(lmap.ravel())[1:]
        drop = np.flatnonzero(cnt != cnt.max()) + 1
        img[np.isin(lmap, drop) & mask] = 0
    return img


def host_decisions(raw, gt, classes):
    """determine_postprocessing's decisions (not advanced, dice_threshold 0) from arrays, with aggregate_scores on arrays"""
    from multitalent_amd.evaluation.evaluator import aggregate_scores

    def dice(preds):
        return aggregate_scores([[p, g] for p, g in zip(preds, gt)], labels=classes)['mean']

    d_raw = dice(raw)
    all_fg = [host_remove(r, [tuple(classes)]) for r in raw]
    d_all = dice(all_fg)
    fwc = []
    k = [str(c) for c in classes]
    if any(d_all[c]['Dice'] > d_raw[c]['Dice'] for c in k) and not any(d_all[c]['Dice'] < d_raw[c]['Dice'] for c in k):
        fwc.append(list(classes))
        src, old = all_fg, d_all
    else:
        src, old = raw, d_raw
    if len(classes) > 1:
        d_pc = dice([host_remove(r, classes) for r in src])
        fwc += [int(c) for c in classes if d_pc[str(c)]['Dice'] > old[str(c)]['Dice']]
    return fwc, host_remove_all(raw, fwc)


def host_remove_all(raw, fwc):
    return [host_remove(r, fwc) for r in raw]


def write_preprocessed_cases(root, plans, n=3, shape=(20, 40, 44), seed=0):
    """<root>/<data_identifier>_stage1/*.npz|pkl plus <root>/gt_segmentations/*.nii.gz, no resampling, one crop offset"""
    from multitalent_amd.utilities.nifti_io import write_image
    rng = np.random.default_rng(seed)
    folder = os.path.join(root, plans['data_identifier'] + '_stage1')
    os.makedirs(folder, exist_ok=True)
    os.makedirs(os.path.join(root, 'gt_segmentations'), exist_ok=True)
    sp = np.array([2.0, 1.0, 1.0])
    for i in range(n):
        key = 'case_%03d' % i
        after = np.array(shape)
        before = after + np.array([2, 3, 1])
        lo = [1, 2, 0]
        seg = np.zeros(shape, np.float32)
        seg[4:14, 6:30, 8:36] = 1
        seg[8:12, 12:22, 14:28] = 2
        data = np.concatenate([rng.standard_normal((1,) + shape).astype(np.float32) + seg[None], seg[None]])
        props = dict(list_of_data_files=['/raw/imagesTr/' + key + '_0000.nii.gz'], original_spacing=sp, spacing_after_resampling=sp,
                     size_after_cropping=after, original_size_of_raw_data=before, crop_bbox=[[lo[j], lo[j] + after[j]] for j in range(3)],
                     itk_spacing=tuple(float(v) for v in sp[::-1]), itk_origin=(0., 0., 0.), itk_direction=tuple(np.eye(3).ravel()),
                     class_locations={1: np.argwhere(seg == 1), 2: np.argwhere(seg == 2)})
        np.savez_compressed(os.path.join(folder, key + '.npz'), data=data)
        with open(os.path.join(folder, key + '.pkl'), 'wb') as f:
            pickle.dump(props, f)
        gt = np.zeros(tuple(before), np.uint8)
        gt[lo[0]:lo[0] + shape[0], lo[1]:lo[1] + shape[1], lo[2]:lo[2] + shape[2]] = seg.astype(np.uint8)
        write_image(gt, os.path.join(root, 'gt_segmentations', key + '.nii.gz'), props['itk_spacing'])


def make_trainer(root, out):
    from multitalent_amd import plans as P
    from multitalent_amd.training.model_restore import find_trainer_class
    sp = {'batch_size': 2, 'patch_size': np.array([16, 32, 32]), 'pool_op_kernel_sizes': [[2, 2, 2], [1, 2, 2]],
          'conv_kernel_sizes': [[3, 3, 3]] * 3, 'do_dummy_2D_data_aug': False, 'current_spacing': np.array([2.0, 1.0, 1.0])}
    plans = P.make_plans(sp, base_num_features=4, num_classes=2, stage=1)
    write_preprocessed_cases(root, plans)
    torch.manual_seed(0)
    tr = find_trainer_class('nnUNetTrainerV2')(plans, 'all', output_folder=out, dataset_directory=root, batch_dice=False, stage=1,
                                               unpack_data=False)
    tr.initialize(False)
    return tr


def test_validate_runs_the_postprocessing_search(tmp_path):
    from multitalent_amd.utilities.nifti_io import read_image
    root = str(tmp_path / 'Task001_Synthetic')
    tr = make_trainer(root, str(tmp_path / 'res'))
    # fold 'all' validates every case; the untrained network's label maps have many components of every class
    tr.validate(do_mirroring=False, save_softmax=False, validation_folder_name='validation_raw', run_postprocessing_on_folds=False)
    vf = os.path.join(tr.output_folder, 'validation_raw')
    ref = {f: read_image(os.path.join(vf, f)) for f in sorted(os.listdir(vf)) if f.endswith('.nii.gz')}
    assert len(ref) == 3
    assert not os.path.exists(os.path.join(tr.output_folder, 'postprocessing.json'))
    assert not os.path.exists(os.path.join(tr.output_folder, 'validation_raw_postprocessed'))
    tr.validate(do_mirroring=False, save_softmax=False, validation_folder_name='validation_raw', run_postprocessing_on_folds=True)
    assert os.path.isfile(os.path.join(tr.output_folder, 'postprocessing.json'))
    assert os.path.isfile(os.path.join(tr.output_folder, 'validation_raw_postprocessed', 'summary.json'))
    assert not os.path.exists(os.path.join(tr.output_folder, 'temp_allClasses'))
    assert not os.path.exists(os.path.join(tr.output_folder, 'temp_perClass'))
    for f, im in ref.items():                                      # validation_raw is what the run without the search wrote
        got = read_image(os.path.join(vf, f))
        assert np.array_equal(np.asarray(got.array), np.asarray(im.array)), f
        assert got.spacing == im.spacing and got.origin == im.origin and got.direction == im.direction
    pp = json.load(open(os.path.join(tr.output_folder, 'postprocessing.json')))
    assert pp['validation_raw'] == 'validation_raw' and pp['validation_final'] == 'validation_raw_postprocessed'
    assert pp['num_samples'] == 3 and pp['min_valid_object_sizes'] == 'None'
    names = sorted(ref)
    raw = [np.asarray(ref[f].array) for f in names]
    gt = [np.asarray(read_image(os.path.join(root, 'gt_segmentations', f)).array) for f in names]
    fwc, final = host_decisions(raw, gt, [1, 2])
    assert pp['for_which_classes'] == fwc
    for f, want in zip(names, final):
        got = np.asarray(read_image(os.path.join(tr.output_folder, 'validation_raw_postprocessed', f)).array)
        assert np.array_equal(got, want), f
    print("validate: for_which_classes", fwc, "components per raw case",
          [int(ndimage.label(r > 0)[1]) for r in raw])


def test_multitalent_trainer_validate_keeps_ignoring_the_flag():
    """MultiTalent_Trainer_DDP.py:129-134: run_postprocessing_on_folds IS IGNORED — the override does not reach the search."""
    import inspect
    from multitalent_amd.training.network_training.custom_trainers.MultiTalent.MultiTalent.MultiTalent_Trainer_DDP import \
        MultiTalent_trainer_ddp
    from multitalent_amd.training.network_training.nnUNetTrainer import nnUNetTrainer
    assert MultiTalent_trainer_ddp.validate is not nnUNetTrainer.validate
    src = inspect.getsource(MultiTalent_trainer_ddp.validate)
    assert 'super().validate' not in src and 'determine_postprocessing' not in src and 'postprocessing.json' not in src
