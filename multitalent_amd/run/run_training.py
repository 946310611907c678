"""`nnUNet_train` (reference run/run_training.py:29-194): one process, one device, for the single-process trainers
(`nnUNetTrainerV2`, `nnUNetTrainerV2_warmupsegheads*`): the readme's fine-tuning command
`nnUNet_train 3d_fullres nnUNetTrainerV2_warmupsegheads TASK FOLD -p PLANS -pretrained_weights CHECKPOINT`.
Flow: configuration -> trainer(plans, fold, ...) WITHOUT a local rank -> initialize -> [continue | pretrained weights] ->
run_training -> validate.  `--find_lr` and `--disable_next_stage_pred` are accepted and ignored, as in `run_training_DDP`
(`3d_lowres` and the cascade are not on this path).  A DDP trainer belongs to `run_training_DDP`."""
import argparse

from ..training.network_training.nnUNetTrainer import nnUNetTrainer, nnUNetTrainerV2_DDP
from .default_configuration import convert_id_to_task_name, default_plans_identifier, get_default_configuration
from .load_pretrained_weights import load_pretrained_weights


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("network")
    ap.add_argument("network_trainer")
    ap.add_argument("task", help="can be task name or task id")
    ap.add_argument("fold", help="0, 1, ..., 5 or 'all'")
    ap.add_argument("-val", "--validation_only", action="store_true", help="only run the validation")
    ap.add_argument("-c", "--continue_training", action="store_true", help="continue a previous training")
    ap.add_argument("-p", default=default_plans_identifier, help="plans identifier")
    ap.add_argument("--use_compressed_data", default=False, action="store_true")
    ap.add_argument("--deterministic", default=False, action="store_true")
    ap.add_argument("--npz", default=False, action="store_true", help="export the softmax of the validation predictions as well")
    ap.add_argument("--find_lr", default=False, action="store_true", help="accepted and ignored")
    ap.add_argument("--valbest", default=False, action="store_true")
    ap.add_argument("--fp32", default=False, action="store_true", help="disable mixed precision training")
    ap.add_argument("--val_folder", default="validation_raw")
    ap.add_argument("--disable_saving", action='store_true')
    ap.add_argument("--disable_postprocessing_on_folds", action='store_true')
    ap.add_argument('--val_disable_overwrite', action='store_false', default=True)
    ap.add_argument('--disable_next_stage_pred', action='store_true', default=False, help="accepted and ignored")
    ap.add_argument('-pretrained_weights', type=str, default=None,
                    help="checkpoint (.model) to start from; only used when a new training starts")
    a = ap.parse_args(argv)
    task = a.task if a.task.startswith("Task") else convert_id_to_task_name(int(a.task))
    fold = a.fold if a.fold == 'all' else int(a.fold)
    plans_file, output_folder_name, dataset_directory, batch_dice, stage, trainer_class = \
        get_default_configuration(a.network, task, a.network_trainer, a.p)
    if trainer_class is None:
        raise RuntimeError("Could not find trainer class in multitalent_amd.training.network_training")
    assert issubclass(trainer_class, nnUNetTrainer), "network_trainer was found but is not derived from nnUNetTrainer"
    if issubclass(trainer_class, nnUNetTrainerV2_DDP):
        raise RuntimeError("%s is a DDP trainer (its constructor takes a local rank): start it with "
                           "multitalent_amd.run.run_training_DDP under torch.distributed.run" % a.network_trainer)
    trainer = trainer_class(plans_file, fold, output_folder=output_folder_name, dataset_directory=dataset_directory,
                            batch_dice=batch_dice, stage=stage, unpack_data=not a.use_compressed_data,
                            deterministic=a.deterministic, fp16=not a.fp32)
    if a.disable_saving:                        # run_training.py:154-160: only a latest checkpoint, in case the training crashes
        trainer.save_final_checkpoint = False
        trainer.save_best_checkpoint = False
        trainer.save_intermediate_checkpoints = True
        trainer.save_latest_only = True
    trainer.initialize(not a.validation_only)
    if not a.validation_only:
        if a.continue_training:                 # -c wins over -pretrained_weights
            trainer.load_latest_checkpoint()
        elif a.pretrained_weights is not None:
            load_pretrained_weights(trainer.network, a.pretrained_weights)
        trainer.run_training()
    elif a.valbest:
        trainer.load_best_checkpoint(train=False)
    else:
        trainer.load_final_checkpoint(train=False)
    trainer.network.eval()
    trainer.validate(save_softmax=a.npz, validation_folder_name=a.val_folder,
                     run_postprocessing_on_folds=not a.disable_postprocessing_on_folds, overwrite=a.val_disable_overwrite)


if __name__ == "__main__":
    main()
