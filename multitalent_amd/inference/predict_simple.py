"""`nnUNet_predict` (reference nnunet/inference/predict_simple.py:25-221): the same flags; the model folder is
`<RESULTS_FOLDER>/nnUNet/<model>/<task>/<trainer>__<plans identifier>` and the work is `predict.predict_from_folder`.  Only the
3D full-resolution and low-resolution configurations exist on this path: `-m 2d` and `-m 3d_cascade_fullres` raise."""
import argparse
import os

from ..run.default_configuration import convert_id_to_task_name, default_plans_identifier, network_training_output_dir

default_trainer = "nnUNetTrainerV2"
default_cascade_trainer = "nnUNetTrainerV2CascadeFullRes"


def build_parser():
    ap = argparse.ArgumentParser(description="Predict every case of a folder with a trained softmax nnU-Net model.")
    ap.add_argument("-i", '--input_folder', required=True, help="CASE_XXXX.nii.gz per modality XXXX (0000, 0001, ...)")
    ap.add_argument('-o', "--output_folder", required=True)
    ap.add_argument('-t', '--task_name', required=True, help="task name (TaskXXX_...) or task id")
    ap.add_argument('-tr', '--trainer_class_name', required=False, default=default_trainer)
    ap.add_argument('-ctr', '--cascade_trainer_class_name', required=False, default=default_cascade_trainer)
    ap.add_argument('-m', '--model', required=False, default="3d_fullres", help="3d_fullres or 3d_lowres")
    ap.add_argument('-p', '--plans_identifier', required=False, default=default_plans_identifier)
    ap.add_argument('-f', '--folds', nargs='+', default='None', help="default: every fold_* of the model folder")
    ap.add_argument('-z', '--save_npz', required=False, action='store_true', help="also store the probabilities, for ensembling")
    ap.add_argument('-l', '--lowres_segmentations', required=False, default='None')
    ap.add_argument("--part_id", type=int, required=False, default=0)
    ap.add_argument("--num_parts", type=int, required=False, default=1)
    ap.add_argument("--num_threads_preprocessing", required=False, default=6, type=int, help="accepted and ignored")
    ap.add_argument("--num_threads_nifti_save", required=False, default=2, type=int, help="accepted and ignored")
    ap.add_argument("--disable_tta", required=False, default=False, action="store_true", help="no mirroring at test time")
    ap.add_argument("--overwrite_existing", required=False, default=False, action="store_true")
    ap.add_argument("--mode", type=str, default="normal", required=False)
    ap.add_argument("--all_in_gpu", type=str, default="None", required=False, help="None, False or True")
    ap.add_argument("--step_size", type=float, default=0.5, required=False)
    ap.add_argument('-chk', required=False, default='model_final_checkpoint', help="checkpoint name")
    ap.add_argument('--disable_mixed_precision', default=False, action='store_true', required=False)
    return ap


def parse_folds(folds):
    if isinstance(folds, list):
        if folds[0] == 'all' and len(folds) == 1:
            return folds
        return [int(i) for i in folds]
    if folds == "None":
        return None
    raise ValueError("Unexpected value for argument folds")


def model_folder(model, task_name, trainer, plans_identifier):
    """`-t` may be a task id; the folder must exist."""
    assert model in ["2d", "3d_lowres", "3d_fullres", "3d_cascade_fullres"], "-m must be 2d, 3d_lowres, 3d_fullres or " \
                                                                             "3d_cascade_fullres"
    if model in ("2d", "3d_cascade_fullres"):
        raise NotImplementedError("-m %s: only the 3D single-stage configurations (3d_fullres, 3d_lowres) are predicted on the device; "
                                  "2D networks and the cascade are not on this path" % model)
    if not task_name.startswith("Task"):
        task_name = convert_id_to_task_name(int(task_name))
    folder = os.path.join(network_training_output_dir(), model, task_name, trainer + "__" + plans_identifier)
    print("using model stored in ", folder)
    assert os.path.isdir(folder), "model output folder not found. Expected: %s" % folder
    return folder


def main(argv=None):
    from .predict import predict_from_folder
    a = build_parser().parse_args(argv)
    folds = parse_folds(a.folds)
    assert a.all_in_gpu in ['None', 'False', 'True']
    all_in_gpu = {'None': None, 'True': True, 'False': False}[a.all_in_gpu]
    folder = model_folder(a.model, a.task_name, a.trainer_class_name, a.plans_identifier)
    predict_from_folder(folder, a.input_folder, a.output_folder, folds, a.save_npz, a.num_threads_preprocessing,
                        a.num_threads_nifti_save, None if a.lowres_segmentations == "None" else a.lowres_segmentations, a.part_id,
                        a.num_parts, not a.disable_tta, overwrite_existing=a.overwrite_existing, mode=a.mode,
                        overwrite_all_in_gpu=all_in_gpu, mixed_precision=not a.disable_mixed_precision, step_size=a.step_size,
                        checkpoint_name=a.chk)


if __name__ == "__main__":
    main()
