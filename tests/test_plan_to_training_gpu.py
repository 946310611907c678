"""Raw files -> trained iteration -> fine-tuning, the chain of the reference's readme at toy size.  Task901_Tiny is planned and
preprocessed by `nnUNet_plan_and_preprocess`, nnUNetTrainerV2 trains two iterations from the result and saves a checkpoint;
Task902_Target (4 cases, labels 0..3, another spacing) is preprocessed with 901's plans (`-overwrite_plans`), and
nnUNetTrainerV2_warmupsegheads starts from 901's checkpoint on it.  Every stage has its own tests against the reference; this file
checks that plans, folders, identifiers, transposes and normalisation constants agree along the chain."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planning_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
SOURCE_PLANS = 'nnUNetPlansv2.1_plans_3D.pkl'


def _trainer(network_trainer, task, plans_identifier):
    from multitalent_amd.run.default_configuration import get_default_configuration
    plans_file, output_folder, dataset_directory, batch_dice, stage, trainer_class = \
        get_default_configuration('3d_fullres', task, network_trainer, plans_identifier)
    tr = trainer_class(plans_file, 'all', output_folder=output_folder, dataset_directory=dataset_directory, batch_dice=batch_dice,
                       stage=stage, unpack_data=True, deterministic=False, fp16=False)
    os.makedirs(tr.output_folder, exist_ok=True)
    tr.initialize(True)
    return tr


@pytest.fixture(scope='module')
def chain(dev, tmp_path_factory):
    e = PC.ToyEnvironment(tmp_path_factory.mktemp('plan_to_training'))
    e.plan_and_preprocess(PC.TASK901, '-pl3d', 'ExperimentPlanner3D_v21', '--verify_dataset_integrity')
    e.source_plans = os.path.join(e.preprocessed, PC.TASK901['name'], SOURCE_PLANS)
    tr = _trainer('nnUNetTrainerV2', PC.TASK901['name'], 'nnUNetPlansv2.1')
    e.source_batch_dice, e.source_stage = tr.batch_dice, tr.stage
    tr.setup_data_generators()
    tr.network.train()
    np.random.seed(901)
    e.source_batch = next(tr.tr_gen)
    e.source_losses = [float(tr.run_iteration(tr.tr_gen, True)) for _ in range(2)]
    e.checkpoint = os.path.join(tr.output_folder, 'model_final_checkpoint.model')
    tr.save_checkpoint(e.checkpoint)
    e.source_patch = tuple(int(i) for i in tr.patch_size)
    e.plan_and_preprocess(PC.TASK902, '-pl3d', 'ExperimentPlanner3D_v21_Pretrained', '-overwrite_plans', e.source_plans,
                          '-overwrite_plans_identifier', 'TINY', '--verify_dataset_integrity')
    yield e
    e.close()


def test_two_iterations_from_the_planned_data(chain):
    plans = PC.load_pickle(chain.source_plans)
    assert chain.source_stage == 0 and chain.source_batch_dice is False                  # one stage
    assert chain.source_patch == tuple(int(i) for i in plans['plans_per_stage'][0]['patch_size'])
    b = chain.source_batch
    assert tuple(b['data'].shape) == (plans['plans_per_stage'][0]['batch_size'], 1) + chain.source_patch
    assert len(chain.source_losses) == 2 and np.isfinite(chain.source_losses).all()
    assert os.path.isfile(chain.checkpoint) and os.path.isfile(chain.checkpoint + '.pkl')


def test_the_target_is_preprocessed_with_the_source_plans(chain, tmp_path):
    from multitalent_amd.preprocessing.preprocessing import GenericPreprocessor
    task = PC.TASK902['name']
    out = os.path.join(chain.preprocessed, task)
    source = PC.load_pickle(chain.source_plans)
    plans = PC.load_pickle(os.path.join(out, 'nnUNetPlans_pretrained_TINY_plans_3D.pkl'))
    assert plans['num_classes'] == 3 != source['num_classes'] and plans['data_identifier'] == 'nnUNetData_pretrained_TINY'
    for k in source:
        if k not in ('num_classes', 'data_identifier'):
            assert PC.encode(plans[k]) == PC.encode(source[k]), k
    target = source['plans_per_stage'][0]['current_spacing']
    pre = GenericPreprocessor(source['normalization_schemes'], source['use_mask_for_norm'], source['transpose_forward'],
                              source['dataset_properties']['intensityproperties'])
    pre.run([target], os.path.join(chain.cropped, task), str(tmp_path), 'by_hand', 2)
    got = PC.load_cases(os.path.join(out, 'nnUNetData_pretrained_TINY_stage0'))
    PC.assert_same_cases(got, PC.load_cases(str(tmp_path / 'by_hand_stage0')))
    assert len(got) == 4
    for k, (a, props) in got.items():
        assert np.array_equal(props['spacing_after_resampling'], target)                 # 901's spacing, not 902's own
        assert a.shape[1:] == PC.expected_shape(props, target, source['transpose_forward'])
        assert sorted(props['class_locations']) == [1, 2, 3]                             # 902's classes
    own = PC.load_pickle(os.path.join(chain.cropped, task, 'dataset_properties.pkl'))['intensityproperties'][0]
    assert own['mean'] != source['dataset_properties']['intensityproperties'][0]['mean']


def test_finetuning_starts_from_the_source_checkpoint(chain):
    from multitalent_amd.run.load_pretrained_weights import load_pretrained_weights
    tr = _trainer('nnUNetTrainerV2_warmupsegheads', PC.TASK902['name'], 'nnUNetPlans_pretrained_TINY')
    assert tr.num_classes == 4 and tuple(int(i) for i in tr.patch_size) == chain.source_patch
    assert tr.folder_with_preprocessed_data.endswith('nnUNetData_pretrained_TINY_stage0')
    before = {k: v.detach().cpu().clone() for k, v in tr.network.state_dict().items()}
    source = torch.load(chain.checkpoint, map_location='cpu', weights_only=False)['state_dict']
    transferred = load_pretrained_weights(tr.network, chain.checkpoint)
    after = {k: v.detach().cpu() for k, v in tr.network.state_dict().items()}
    heads = [k for k in before if k.startswith('seg_outputs')]
    assert len(heads) > 0 and sorted(transferred) == sorted(k for k in before if k not in heads)
    assert all(k in transferred for k in before if 'conv_blocks' in k)
    assert all(torch.equal(after[k], source[k].cpu()) for k in transferred)
    assert all(torch.equal(after[k], before[k]) and after[k].shape != source[k].shape for k in heads)        # 4 classes against 3
    tr.setup_data_generators()
    tr.network.train()
    tr.epoch = 0
    tr.maybe_update_lr()
    assert np.isfinite(float(tr.run_iteration(tr.tr_gen, True)))
