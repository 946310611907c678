"""The stock prediction chain of a softmax model against the REAL reference's output (part (c) of tests/golden/ensemble.npz,
tools/oracle_gen/make_golden_ensemble.py): `inference.predict.predict_cases` with a two-fold `nnUNetTrainerV2` model, `save_npz`
and a `postprocessing.json` in the model folder; `predict_simple.main` on the same folders; `consolidate_folds`.

The masks are compared with tests/mask_check.py: identical away from ties of the reference's float32 probabilities, the decision
rule of their own probabilities everywhere, and the number of tie voxels equals the count the generator recorded."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
TASK, TRAINER, PLANS_ID = 'Task555_Tiny', 'nnUNetTrainerV2', 'nnUNetPlansv2.1'


def golden():
    return np.load(os.path.join(HERE, 'golden', 'ensemble.npz')), json.load(open(os.path.join(HERE, 'golden', 'ensemble.json')))['c']


def plans(meta):
    from multitalent_amd import plans as P
    sp = {'batch_size': 2, 'patch_size': np.array([8, 16, 16]), 'pool_op_kernel_sizes': [[2, 2, 2], [1, 2, 2]],
          'conv_kernel_sizes': [[3, 3, 3]] * 3, 'do_dummy_2D_data_aug': False, 'current_spacing': np.array([2.0, 1.0, 1.0])}
    p = P.make_plans(sp, base_num_features=4, num_classes=2, stage=1)
    p['dataset_properties'] = {'intensityproperties': {0: dict(meta['predict']['intensityproperties'])}}
    return p


@pytest.fixture(scope='module')
def predicted(tmp_path_factory):
    """The model folder (two folds with the golden weights, postprocessing.json), the input folder, and ONE predict_cases run whose
    float32 probabilities and raw mask are captured on the way to the export."""
    import multitalent_amd.inference.segmentation_export as se
    from multitalent_amd.inference.predict import predict_cases
    from multitalent_amd.training.model_restore import find_trainer_class
    from multitalent_amd.utilities.nifti_io import write_image
    z, meta = golden()
    root = tmp_path_factory.mktemp('softmax')
    model = str(root / 'res' / 'nnUNet' / '3d_fullres' / TASK / (TRAINER + '__' + PLANS_ID))
    P = plans(meta)
    sd0 = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('c/sd0/')}
    sd1 = dict(sd0, **{k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('c/sd1/')})
    assert any(not torch.equal(sd0[k], sd1[k]) for k in sd0)
    for fold, sd in ((0, sd0), (1, sd1)):
        tr = find_trainer_class(TRAINER)(P, fold, output_folder=model, dataset_directory=None, stage=1, unpack_data=False, fp16=False)
        tr.initialize(False)
        tr.network.load_state_dict(sd, strict=True)
        tr.network.engine().mark_params_dirty()
        tr.save_checkpoint(os.path.join(tr.output_folder, 'model_final_checkpoint.model'))
    with open(os.path.join(model, 'plans.pkl'), 'wb') as f:
        pickle.dump(P, f)
    json.dump(meta['predict']['postprocessing'], open(os.path.join(model, 'postprocessing.json'), 'w'))
    m = meta['predict']
    inp, outp = root / 'in', root / 'out'
    inp.mkdir()
    write_image(z['c/raw/vol'], str(inp / (m['case'] + '_0000.nii.gz')), tuple(float(i) for i in m['spacing_zyx'][::-1]), tuple(m['origin']))
    captured = {}
    real = se.save_segmentation_nifti_from_softmax

    def capture(softmax, *a, **k):
        captured['probs'] = softmax.detach().float().cpu().numpy().copy()
        captured['seg'] = np.array(real(softmax, *a, **k), copy=True)
        return captured['seg']

    se.save_segmentation_nifti_from_softmax = capture
    try:
        predict_cases(model, [[str(inp / (m['case'] + '_0000.nii.gz'))]], [str(outp / (m['case'] + '.nii.gz'))], [0, 1], True, 1, 1, None,
                      True, mixed_precision=False, overwrite_existing=True, all_in_gpu=False, step_size=0.5,
                      checkpoint_name='model_final_checkpoint')
    finally:
        se.save_segmentation_nifti_from_softmax = real
    return dict(z=z, meta=m, root=root, model=model, inp=str(inp), out=str(outp), **captured)


def test_predict_cases_matches_reference(predicted):
    from mask_check import check_masks
    from multitalent_amd.utilities.nifti_io import read_image
    z, m, out = predicted['z'], predicted['meta'], predicted['out']
    ref_probs, ref_seg = z['c/probs'], z['c/seg']
    probs, seg = predicted['probs'], predicted['seg']
    assert probs.shape == ref_probs.shape and seg.shape == ref_seg.shape == tuple(m['shape']) and seg.dtype == np.uint8
    bb = m['crop_bbox']
    box = tuple(slice(b[0], b[1]) for b in bb)
    outside = np.ones(seg.shape, bool)
    outside[box] = False
    assert not seg[outside].any() and not ref_seg[outside].any()
    ties, ndiff = check_masks(seg[box], ref_seg[box], probs, ref_probs, None, 1e-4, 'predict_cases %s' % m['case'], live=True)
    assert ties == m['ties_1e-4'] and probs[0].size == m['voxels']
    print("predict_cases: max |p - p_ref| = %.3e" % float(np.abs(probs - ref_probs).max()))
    # stored probabilities (float16) and properties
    stored = np.load(os.path.join(out, m['case'] + '.npz'))['softmax']
    assert stored.dtype == np.float16 and stored.shape == z['c/npz'].shape
    err = float(np.abs(stored.astype(np.float32) - z['c/npz'].astype(np.float32)).max())
    print("predict_cases: stored probabilities, max |p - p_ref| = %.3e" % err)
    assert err < 1e-3
    props = pickle.load(open(os.path.join(out, m['case'] + '.pkl'), 'rb'))
    assert [int(i) for i in props['size_after_cropping']] == m['size_after_cropping']
    assert [[int(j) for j in i][0] for i in props['crop_bbox']] == [b[0] for b in bb]
    # the postprocessed mask is what is on disk, with the input's geometry; the json travels with it
    assert json.load(open(os.path.join(out, 'postprocessing.json'))) == m['postprocessing']
    img = read_image(os.path.join(out, m['case'] + '.nii.gz'))
    final = np.asarray(img.array)
    assert np.allclose(img.spacing, m['spacing_zyx'][::-1], rtol=1e-6) and np.allclose(img.origin, m['origin'])
    assert final.shape == seg.shape and int((final != seg).sum()) > 0, "the postprocessing must have removed something"
    assert not (final[final != seg]).any(), "postprocessing only removes"
    if ndiff == 0:
        assert np.array_equal(final, z['c/seg_pp'])


def test_overwrite_existing_false_skips_finished_cases(predicted):
    from multitalent_amd.inference.predict import predict_cases
    m, out = predicted['meta'], predicted['out']
    files = [os.path.join(out, m['case'] + e) for e in ('.nii.gz', '.npz')]
    before = [os.stat(f).st_mtime_ns for f in files]
    predict_cases(predicted['model'], [[os.path.join(predicted['inp'], m['case'] + '_0000.nii.gz')]], [files[0]], [0, 1], True, 1, 1, None,
                  True, mixed_precision=False, overwrite_existing=False, disable_postprocessing=True)
    assert [os.stat(f).st_mtime_ns for f in files] == before


def test_predict_simple_gives_the_same_files(predicted, monkeypatch):
    from multitalent_amd.inference.predict_simple import main
    from multitalent_amd.utilities.nifti_io import read_image
    m = predicted['meta']
    monkeypatch.setenv('RESULTS_FOLDER', str(predicted['root'] / 'res'))
    out2 = str(predicted['root'] / 'out_simple')
    main(['-i', predicted['inp'], '-o', out2, '-t', TASK, '-tr', TRAINER, '-m', '3d_fullres', '-f', '0', '1', '-z',
          '--disable_mixed_precision', '--overwrite_existing'])
    assert {m['case'] + '.nii.gz', m['case'] + '.npz', m['case'] + '.pkl', 'plans.pkl', 'postprocessing.json'} <= set(os.listdir(out2))
    a, b = read_image(os.path.join(predicted['out'], m['case'] + '.nii.gz')), read_image(os.path.join(out2, m['case'] + '.nii.gz'))
    assert np.array_equal(np.asarray(a.array), np.asarray(b.array)) and np.allclose(a.spacing, b.spacing) and np.allclose(a.origin, b.origin)
    pa, pb = (np.load(os.path.join(o, m['case'] + '.npz'))['softmax'] for o in (predicted['out'], out2))
    assert np.array_equal(pa.view(np.uint16), pb.view(np.uint16))


def test_consolidate_folds_matches_reference(tmp_path):
    from multitalent_amd.evaluation.evaluator import aggregate_scores
    from multitalent_amd.postprocessing.consolidate_postprocessing import consolidate_folds
    from multitalent_amd.utilities.nifti_io import read_image, write_image
    z, meta = golden()
    m = meta['consolidate']
    base = str(tmp_path / 'cv')
    sp = tuple(float(i) for i in m['spacing_zyx'][::-1])
    os.makedirs(os.path.join(base, 'gt_niftis'))
    for fold, cases in m['folds'].items():
        vf = os.path.join(base, 'fold_%s' % fold, 'validation_raw')
        os.makedirs(vf)
        pairs = []
        for c in cases:
            write_image(z['c/cv/%s/%s/raw' % (fold, c)], os.path.join(vf, c + '.nii.gz'), sp)
            write_image(z['c/cv/%s/%s/gt' % (fold, c)], os.path.join(base, 'gt_niftis', c + '.nii.gz'), sp)
            pairs.append((os.path.join(vf, c + '.nii.gz'), os.path.join(base, 'gt_niftis', c + '.nii.gz')))
        aggregate_scores(pairs, labels=[0, 1, 2], json_output_file=os.path.join(vf, 'summary.json'))
    consolidate_folds(base, folds=(0, 1))
    assert sorted(os.listdir(base)) == m['folders']
    pp = json.load(open(os.path.join(base, 'postprocessing.json')))
    ref = m['postprocessing']
    assert pp['for_which_classes'] == ref['for_which_classes'] and pp['min_valid_object_sizes'] == ref['min_valid_object_sizes']
    assert pp['num_samples'] == ref['num_samples'] == 4
    for sub, dice in m['dice'].items():
        mean = json.load(open(os.path.join(base, sub, 'summary.json')))['results']['mean']
        assert sorted(mean) == sorted(dice)
        for c, d in dice.items():
            assert abs(mean[c]['Dice'] - d) <= 1e-12, (sub, c, mean[c]['Dice'], d)
    for cases in m['folds'].values():
        for c in cases:
            got = np.asarray(read_image(os.path.join(base, 'cv_niftis_postprocessed', c + '.nii.gz')).array)
            assert np.array_equal(got, z['c/cv/final/' + c]), c
