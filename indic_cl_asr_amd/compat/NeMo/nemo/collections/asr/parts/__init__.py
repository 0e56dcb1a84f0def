"""`nemo.collections.asr.parts` names the CL scripts and NeMo configs reach."""
