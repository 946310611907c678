"""The folders of a task (reference nnunet/paths.py:19-60), read from the reference's environment variables each time they are
asked for, so that a test or a driver may set them after the import:

  nnUNet_raw_data_base   -> `nnUNet_raw_data()` = <base>/nnUNet_raw_data and `nnUNet_cropped_data()` = <base>/nnUNet_cropped_data
  nnUNet_preprocessed    -> `preprocessing_output_dir()`
  RESULTS_FOLDER         -> `network_training_output_dir()` = <folder>/nnUNet

Each function returns None where its variable is not set (the reference's module constants are None then); `require` turns that
into an error that names the variable.  `run/default_configuration.py` keeps its own two functions, which raise."""
import os

default_data_identifier = 'nnUNetData_plans_v2.1'
my_output_identifier = "nnUNet"
default_num_threads = 8


def base():
    return os.environ.get('nnUNet_raw_data_base')


def nnUNet_raw_data():
    b = base()
    return os.path.join(b, "nnUNet_raw_data") if b is not None else None


def nnUNet_cropped_data():
    b = base()
    return os.path.join(b, "nnUNet_cropped_data") if b is not None else None


def preprocessing_output_dir():
    return os.environ.get('nnUNet_preprocessed')


def network_training_output_dir_base():
    return os.environ.get('RESULTS_FOLDER')


def network_training_output_dir():
    b = network_training_output_dir_base()
    return os.path.join(b, my_output_identifier) if b is not None else None


_VARIABLE = {'nnUNet_raw_data': 'nnUNet_raw_data_base', 'nnUNet_cropped_data': 'nnUNet_raw_data_base',
             'preprocessing_output_dir': 'nnUNet_preprocessed', 'network_training_output_dir': 'RESULTS_FOLDER'}


def require(fn):
    """fn: one of the folder functions above -> its folder, or RuntimeError naming the environment variable that is missing."""
    d = fn()
    if d is None:
        raise RuntimeError("%s is not defined: set it as the reference's paths.py describes" % _VARIABLE[fn.__name__])
    return d
