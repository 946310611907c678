"""Host side of the elastic deformation and MaskTransform of the device augmentation chain (no GPU): which draws
SpatialTransformDevice.draw() takes from numpy's stream, MaskTransformDevice against batchgenerators' loop written out, and the
parameters on their way from default_3d_augmentation_params through the trainer."""
import numpy as np
import torch


def _hand_drawn_default(st):
    """the draws SpatialTransformDevice.draw() has always made for its default configuration (rotation and scaling with probability
    1, every axis rotated, one scale for all axes, centre crop), written out: returns the matrix."""
    from multitalent_amd.training.data_augmentation.spatial import rotation_matrix_3d
    assert np.random.uniform() < st.p_rot
    a = []
    for lo, hi in st.angles:
        assert np.random.uniform() <= st.p_rot_axis
        a.append(np.random.uniform(lo, hi))
    m = rotation_matrix_3d(*a)
    assert np.random.uniform() < st.p_scale
    if np.random.random() < 0.5 and st.scale[0] < 1:
        sc = np.random.uniform(st.scale[0], 1)
    else:
        sc = np.random.uniform(max(st.scale[0], 1), st.scale[1])
    return np.full(3, sc)[:, None] * m


def test_draw_without_elastic_consumes_the_stream_it_always_did():
    from multitalent_amd.training.data_augmentation.spatial import SpatialTransformDevice
    st = SpatialTransformDevice((12, 20, 20))
    np.random.seed(7)
    m, ctr, modified = st.draw((20, 30, 30))
    nxt = np.random.uniform()
    np.random.seed(7)
    m_hand = _hand_drawn_default(st)
    assert np.random.uniform() == nxt
    assert modified and np.array_equal(m, m_hand) and np.array_equal(ctr, [9.5, 14.5, 14.5])
    assert st._drawn_elastic is None


def test_elastic_draw_comes_first():
    from multitalent_amd.training.data_augmentation.spatial import SpatialTransformDevice
    # p_el = 0: exactly one extra uniform, before the rotation draw
    st = SpatialTransformDevice((12, 20, 20), do_elastic_deform=True, p_el_per_sample=0)
    np.random.seed(8)
    m, _, _ = st.draw((20, 30, 30))
    nxt = np.random.uniform()
    np.random.seed(8)
    np.random.uniform()
    m_hand = _hand_drawn_default(st)
    assert np.random.uniform() == nxt and np.array_equal(m, m_hand) and st._drawn_elastic is None
    # p_el = 1: u, alpha, sigma, one integer seed, then the rotation
    st = SpatialTransformDevice((12, 20, 20), do_elastic_deform=True, p_el_per_sample=1, alpha=(100., 300.), sigma=(3., 5.),
                                do_rotation=False, do_scale=False)
    np.random.seed(9)
    m, ctr, modified = st.draw((20, 30, 30))
    nxt = np.random.uniform()
    np.random.seed(9)
    np.random.uniform()
    a, s = np.random.uniform(100., 300.), np.random.uniform(3., 5.)
    seed = int(np.random.randint(0, 2 ** 31 - 1))
    assert np.random.uniform() == nxt
    assert st._drawn_elastic == (a, s, seed)
    assert modified and np.array_equal(m, np.eye(3))          # a deformed sample takes the interpolating path
    # batchgenerators' defaults, appended at the end of the signature
    st = SpatialTransformDevice((12, 20, 20))
    assert st.alpha == (0., 1000.) and st.sigma == (10., 13.) and st.do_elastic is False


def test_mask_transform_matches_the_loop():
    from multitalent_amd.training.data_augmentation.color import MaskTransformDevice
    rs = np.random.RandomState(0)
    data = rs.randn(3, 3, 4, 5, 6).astype(np.float32)
    seg = rs.randint(-1, 3, size=(3, 2, 4, 5, 6)).astype(np.float32)
    for dct, idx, outside in (({0: True, 1: False, 2: True}, 0, 0), ({0: False, 1: True, 2: False}, 1, -7.5)):
        ref = data.copy()
        for b in range(data.shape[0]):
            for c in range(data.shape[1]):
                if dct[c]:
                    ref[b, c][seg[b, idx] < 0] = outside
        t = torch.from_numpy(data.copy())
        got = MaskTransformDevice(dct, mask_idx_in_seg=idx, set_outside_to=outside)(t, torch.from_numpy(seg))
        assert got is t and np.array_equal(got.numpy(), ref)
        assert (ref != data).any() and all(np.array_equal(ref[:, c], data[:, c]) for c in dct if not dct[c])
    t = torch.from_numpy(data.copy())
    assert np.array_equal(MaskTransformDevice({0: False, 1: False, 2: False})(t, torch.from_numpy(seg)).numpy(), data)


def test_parameters_reach_the_chain(tmp_path):
    from multitalent_amd import plans as P
    from multitalent_amd.training.data_augmentation.color import default_3d_augmentation_params
    from multitalent_amd.training.model_restore import find_trainer_class
    p = default_3d_augmentation_params()
    assert p['elastic_deform_alpha'] == (0., 900.) and p['elastic_deform_sigma'] == (9., 13.)
    assert p['do_elastic'] is False and p['p_eldef'] == 0.2

    class ElasticTrainer(find_trainer_class('nnUNetTrainerV2')):
        def setup_augmentation_params(self):
            q = super().setup_augmentation_params()
            q['do_elastic'] = True
            self.data_aug_params.update(q)
            return q

    for dummy_2d, alpha in ((False, (0., 900.)), (True, (0., 200.))):
        sp = {'batch_size': 2, 'patch_size': np.array([12, 24, 24]), 'pool_op_kernel_sizes': [[2, 2, 2], [2, 2, 2]],
              'conv_kernel_sizes': [[3, 3, 3]] * 3, 'do_dummy_2D_data_aug': dummy_2d}
        plans = P.make_plans(sp, base_num_features=8, num_classes=3, stage=1)
        plans['use_mask_for_norm'] = {0: True}
        tr = ElasticTrainer(plans, 0, output_folder=None, dataset_directory=str(tmp_path), stage=1)
        tr.load_plans_file(); tr.process_plans(tr.plans)
        q = tr.setup_augmentation_params()
        assert q['do_elastic'] is True and q['elastic_deform_alpha'] == alpha and q['elastic_deform_sigma'] == (9., 13.)
        assert q['mask_was_used_for_normalization'] == {0: True} and bool(q['dummy_2D']) is dummy_2d
        assert tr.data_aug_params['do_elastic'] is True
    # the stock trainer leaves it off
    tr = find_trainer_class('nnUNetTrainerV2')(plans, 0, output_folder=None, dataset_directory=str(tmp_path), stage=1)
    tr.load_plans_file(); tr.process_plans(tr.plans)
    assert tr.setup_augmentation_params()['do_elastic'] is False
