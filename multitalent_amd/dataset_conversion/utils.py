"""`generate_dataset_json` and `get_identifiers_from_splitted_files` (reference nnunet/dataset_conversion/utils.py:22-76): the
`dataset.json` of a raw task from the files of its imagesTr / imagesTs folders.  Host code."""
import json
import os

import numpy as np


def get_identifiers_from_splitted_files(folder):
    """The sorted unique case identifiers of a folder of `<case>_XXXX.nii.gz` files (np.unique of the names without their
    last 12 characters)."""
    files = [f for f in os.listdir(folder) if f.endswith('.nii.gz') and os.path.isfile(os.path.join(folder, f))]
    return np.unique([f[:-12] for f in files])


def generate_dataset_json(output_file, imagesTr_dir, imagesTs_dir, modalities, labels, dataset_name, sort_keys=True,
                          license="hands off!", dataset_description="", dataset_reference="", dataset_release='0.0'):
    """output_file: `<task folder>/dataset.json`; imagesTs_dir may be None; modalities: names in the order of `_0000`, `_0001`, ...;
    labels: {int: name} with 0 the background.  Writes the reference's keys (`licence` is spelt as there)."""
    train_identifiers = get_identifiers_from_splitted_files(imagesTr_dir)
    test_identifiers = get_identifiers_from_splitted_files(imagesTs_dir) if imagesTs_dir is not None else []
    json_dict = {}
    json_dict['name'] = dataset_name
    json_dict['description'] = dataset_description
    json_dict['tensorImageSize'] = "4D"
    json_dict['reference'] = dataset_reference
    json_dict['licence'] = license
    json_dict['release'] = dataset_release
    json_dict['modality'] = {str(i): modalities[i] for i in range(len(modalities))}
    json_dict['labels'] = {str(i): labels[i] for i in labels.keys()}
    json_dict['numTraining'] = len(train_identifiers)
    json_dict['numTest'] = len(test_identifiers)
    json_dict['training'] = [{'image': "./imagesTr/%s.nii.gz" % i, "label": "./labelsTr/%s.nii.gz" % i} for i in train_identifiers]
    json_dict['test'] = ["./imagesTs/%s.nii.gz" % i for i in test_identifiers]
    if not output_file.endswith("dataset.json"):
        print("WARNING: output file name is not dataset.json! This may be intentional or not. You decide. Proceeding anyways...")
    with open(output_file, 'w') as f:
        json.dump(json_dict, f, sort_keys=sort_keys, indent=4)
