"""`from nemo.collections.asr.parts.preprocessing.perturb import process_augmentations, AudioAugmentor, ...`
(A/parts/preprocessing/perturb.py): the device-side perturbations of indic_cl_asr_amd.augment under the reference's module
path."""
from indic_cl_asr_amd.augment import (AudioAugmentor, GainPerturbation, Perturbation, ShiftPerturbation,  # noqa: F401
                                      SpeedPerturbation, WhiteNoisePerturbation, perturbation_types,
                                      process_augmentations)
