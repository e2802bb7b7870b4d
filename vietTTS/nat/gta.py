"""vietTTS/nat/gta.py:28-82 — forward_fn / generate_gta: ground-truth-aligned mels from the teacher-forced acoustic model, which runs in
the HIP library (include/vtts_nat.h).  Corpus loading stays with the caller: generate_gta consumes an iterator of (names, batch)."""
from viettts_amd.nat.gta import AcousticInput, forward_fn, generate_gta  # noqa: F401
