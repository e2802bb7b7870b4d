"""vietTTS/hifigan/torch_model.py:221-414 — same module path, names and call signatures for the discriminators and the three losses;
they run, forward only, in the HIP library (viettts_amd/hifigan/torch_model.py)."""
from viettts_amd.hifigan.torch_model import (  # noqa: F401
    LRELU_SLOPE,
    MultiPeriodDiscriminator,
    MultiScaleDiscriminator,
    discriminator_loss,
    feature_loss,
    generator_loss,
    use_discriminators,
)
