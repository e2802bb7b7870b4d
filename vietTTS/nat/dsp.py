"""vietTTS/nat/dsp.py:104-128 — MelFilter with the reference's constructor signature; the transform runs in the HIP library
(include/vtts_mel.h)."""
from viettts_amd.nat.dsp import MelFilter  # noqa: F401
