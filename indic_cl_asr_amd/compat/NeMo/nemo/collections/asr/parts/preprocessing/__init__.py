"""`nemo.collections.asr.parts.preprocessing`: the waveform perturbations."""
