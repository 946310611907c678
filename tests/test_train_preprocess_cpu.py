"""Host side of the training-case pre-processing (no GPU): the rank generator of `class_locations` against the golden of
tools/oracle_gen/make_golden_train_preprocess.py, the reference's signatures, and the loud failure without a device."""
import inspect
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_preprocess.npz')


def test_rank_generator_reproduces_the_golden_locations():
    from multitalent_amd.preprocessing.device_preprocessing import draw_class_ranks
    z = np.load(G)
    all_classes = [int(c) for c in z['all_classes']]
    largest = 0
    for name in z['names']:
        seg = z[name + '/out'][-1]
        locs = [np.argwhere(seg == c) for c in all_classes]
        ranks = draw_class_ranks([len(l) for l in locs])
        for c, l, r in zip(all_classes, locs, ranks):
            want = z['%s/loc%d' % (name, c)]
            if len(l) == 0:
                assert r is None and len(want) == 0
                continue
            assert len(r) == max(min(10000, len(l)), int(np.ceil(0.01 * len(l)))) and len(set(r.tolist())) == len(r)
            assert np.array_equal(l[r], want)
            largest = max(largest, len(l))
    assert largest > 10000                                                  # the golden holds a class beyond the sample cap


def test_rank_generator_one_percent_rule():
    from multitalent_amd.preprocessing.device_preprocessing import draw_class_ranks
    ranks = draw_class_ranks([0, 5, 1500001])
    assert ranks[0] is None and sorted(ranks[1].tolist()) == [0, 1, 2, 3, 4] and len(ranks[2]) == 15001
    rndst = np.random.RandomState(1234)
    assert np.array_equal(ranks[1], rndst.choice(5, 5, replace=False))
    assert np.array_equal(ranks[2], rndst.choice(1500001, 15001, replace=False))


def test_signatures_are_the_references():
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    assert list(inspect.signature(GenericPreprocessor._run_internal).parameters) == [
        'self', 'target_spacing', 'case_identifier', 'output_folder_stage', 'cropped_output_dir', 'force_separate_z', 'all_classes']
    run = inspect.signature(GenericPreprocessor.run).parameters
    assert list(run) == ['self', 'target_spacings', 'input_folder_with_cropped_npz', 'output_folder', 'data_identifier', 'num_threads',
                         'force_separate_z']
    assert run['force_separate_z'].default is None
    assert list(inspect.signature(GenericPreprocessor.load_cropped).parameters) == ['cropped_output_dir', 'case_identifier']
    assert list(inspect.signature(GenericPreprocessor.preprocess_training_case).parameters) == [
        'self', 'data', 'seg', 'properties', 'target_spacing', 'all_classes', 'force_separate_z']


def test_no_device_fails_loudly(tmp_path, monkeypatch):
    import torch
    from multitalent_amd import ops
    from multitalent_amd.preprocessing import device_preprocessing as dp
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    g = GenericPreprocessor({0: 'nonCT'}, {0: True}, [0, 1, 2], None)
    data, seg = np.zeros((1, 4, 5, 6), dtype=np.float32), np.zeros((1, 4, 5, 6), dtype=np.float32)
    props = {'original_spacing': np.array([1.0, 1.0, 1.0])}
    msg = "HIP device only; there is no CPU fallback"
    with pytest.raises(RuntimeError, match=msg):
        g._run_internal(np.array([1.0, 1.0, 1.0]), 'case', str(tmp_path), str(tmp_path), None, [1])
    with pytest.raises(RuntimeError, match=msg):
        g.run([[1.0, 1.0, 1.0]], str(tmp_path), str(tmp_path / 'out'), 'plans')
    with pytest.raises(RuntimeError, match=msg):
        g.preprocess_training_case(data, seg, props, np.array([1.0, 1.0, 1.0]), [1])
    with pytest.raises(RuntimeError, match=msg):
        g.resample_and_normalize(data, np.array([1.0, 1.0, 1.0]), props, seg)
    with pytest.raises(RuntimeError, match=msg):
        dp.resample_seg(torch.zeros(1, 4, 5, 6), (5, 6, 7))
    for call in (lambda: ops.masked_moments(torch.zeros(1, 8)), lambda: ops.intensity_normalize(torch.zeros(8)),
                 lambda: ops.label_counts(torch.zeros(2, 2, 2), [1])):
        with pytest.raises(RuntimeError, match=msg):
            call()
    assert not os.path.exists(tmp_path / 'out')
