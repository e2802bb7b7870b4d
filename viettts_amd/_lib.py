"""ctypes binding of include/vtts_hifigan.h.

The product path has NO CPU fallback: if the shared library is missing or a call fails, a
:class:`VttsError` (or ``OSError`` from the loader) propagates.  Build the library with
``python -m viettts_amd.csrc.build`` (``__graft_entry__.build()`` does).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

ABI_VERSION = 2
MAX_UPSAMPLES = 8
MAX_KERNELS = 4

VTTS_F32 = 0
VTTS_BF16 = 1
VTTS_BF16X3 = 2

STATUS_NAMES = {
    0: "VTTS_OK",
    -1: "VTTS_ERR_INVALID",
    -2: "VTTS_ERR_STATE",
    -3: "VTTS_ERR_MISSING",
    -4: "VTTS_ERR_HIP",
    -5: "VTTS_ERR_NOMEM",
    -6: "VTTS_ERR_SHAPE",
}

# include/vtts_disc.h: the loss buffer's layout
DISC_NUM_FMAPS = 54
DISC_NUM_DISCS = 8
DISC_MIN_SAMPLES = 11
DISC_LOSS_REAL, DISC_LOSS_FAKE, DISC_LOSS_GEN, DISC_LOSS_TOTALS, DISC_LOSS_RESULTS = 54, 62, 70, 78, 128
DISC_LOSS_FLOATS = DISC_LOSS_RESULTS + 2 * (DISC_NUM_FMAPS + 3 * DISC_NUM_DISCS) * 64

VTTS_AUDIO_F32 = 0
VTTS_AUDIO_PCM16 = 1
AUDIO_OUT_PER_BLOCK = 1024  # include/vtts_audio.h: VTTS_AUDIO_OUT_PER_BLOCK
AUDIO_ZEROS = 24  # include/vtts_audio.h: VTTS_AUDIO_ZEROS
AUDIO_BETA = 10.0  # include/vtts_audio.h: VTTS_AUDIO_BETA
AUDIO_MAX_R = 2048  # include/vtts_audio.h: VTTS_AUDIO_MAX_R

VTTS_MEL_F32 = 0
VTTS_MEL_PCM16 = 1
MEL_FRAMES_PER_BLOCK = 8  # include/vtts_mel.h: VTTS_MEL_FRAMES_PER_BLOCK
MEL_MIN_SAMPLES = 385  # include/vtts_mel.h: VTTS_MEL_MIN_SAMPLES

DTW_MAX_FEAT = 128  # include/vtts_dtw.h: VTTS_DTW_MAX_FEAT
DTW_MAX_FRAMES = 4096  # include/vtts_dtw.h: VTTS_DTW_MAX_FRAMES

MCD_MAX_MELS, MCD_MAX_CEPS = 128, 64  # include/vtts_mcd.h: VTTS_MCD_MAX_MELS / _MAX_CEPS
MCD_FRAMES_PER_BLOCK = 64  # include/vtts_mcd.h: VTTS_MCD_FRAMES_PER_BLOCK
MCD_ALPHA = 6.141851463713754  # include/vtts_mcd.h: VTTS_MCD_ALPHA = 10 sqrt(2) / ln 10

PITCH_FRAMES_PER_BLOCK = 8  # include/vtts_pitch.h: VTTS_PITCH_FRAMES_PER_BLOCK
PITCH_MAX_LAG = 512  # include/vtts_pitch.h: VTTS_PITCH_MAX_LAG

LOUDNESS_CHUNK = 32  # include/vtts_loudness.h: VTTS_LOUDNESS_CHUNK
LOUDNESS_SEGMENT = 8192  # include/vtts_loudness.h: VTTS_LOUDNESS_SEGMENT
LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE = 8000, 96000  # include/vtts_loudness.h: VTTS_LOUDNESS_MIN_RATE / _MAX_RATE

STOI_MAX_SAMPLES = 1 << 24  # include/vtts_stoi.h: VTTS_STOI_MAX_SAMPLES
STOI_FRAMES_PER_BLOCK = 8  # include/vtts_stoi.h: VTTS_STOI_FRAMES_PER_BLOCK
STOI_FRAME, STOI_HOP, STOI_BANDS, STOI_SEG = 256, 128, 15, 30  # include/vtts_stoi.h: VTTS_STOI_FRAME / _HOP / _BANDS / _SEG

SPECTRAL_MAX_SAMPLES = 1 << 24  # include/vtts_spectral.h: VTTS_SPECTRAL_MAX_SAMPLES
SPECTRAL_N_FFT = (256, 512, 1024, 2048)  # include/vtts_spectral.h: the transform lengths create() accepts
SPECTRAL_MAX_FRAMES_PER_BLOCK, SPECTRAL_MAX_FRAMES_PER_BLOCK_2048 = 8, 4  # include/vtts_spectral.h: VTTS_SPECTRAL_MAX_FRAMES_PER_BLOCK[_2048]
SPECTRAL_LDS_BUDGET = 81920  # include/vtts_spectral.h: VTTS_SPECTRAL_LDS_BUDGET

VTTS_STFT_CENTER, VTTS_STFT_MEL = 0, 1  # include/vtts_stft.h: the framings
STFT_MAX_SAMPLES = 1 << 24  # include/vtts_stft.h: VTTS_STFT_MAX_SAMPLES
STFT_NOLA_FLOOR = 1e-11  # include/vtts_stft.h: VTTS_STFT_NOLA_FLOOR
DENOISE_MAX_SAMPLES = 1 << 24  # include/vtts_denoise.h: VTTS_DENOISE_MAX_SAMPLES
DENOISE_NOLA_FLOOR = 1e-11  # include/vtts_denoise.h: VTTS_DENOISE_NOLA_FLOOR

LIMITER_TILE = 4096  # include/vtts_limiter.h: VTTS_LIMITER_TILE
LIMITER_RUN = 16  # include/vtts_limiter.h: VTTS_LIMITER_RUN
LIMITER_PHASE_TAPS = 52  # include/vtts_limiter.h: VTTS_LIMITER_PHASE_TAPS
LIMITER_MIN_RATE, LIMITER_MAX_RATE = 8000, 96000  # include/vtts_limiter.h: VTTS_LIMITER_MIN_RATE / _MAX_RATE
LIMITER_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/limiter.hip: the rows whose lengths one launch carries
AUDIO_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/audio.hip, likewise: ROWS_PER_LAUNCH
MEL_ROWS_PER_LAUNCH = 256  # viettts_amd/csrc/mel.hip
PITCH_ROWS_PER_LAUNCH = 256  # viettts_amd/csrc/pitch.hip
STOI_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/stoi.hip
LOUDNESS_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/loudness.hip
SPECTRAL_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/spectral.hip; include/vtts_spectral.h: VTTS_SPECTRAL_ROWS_PER_LAUNCH
STFT_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/stft.hip; include/vtts_stft.h: VTTS_STFT_ROWS_PER_LAUNCH
DENOISE_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/denoise.hip; include/vtts_denoise.h: VTTS_DENOISE_ROWS_PER_LAUNCH
DTW_PAIRS_PER_LAUNCH = 128  # viettts_amd/csrc/dtw.hip: PAIRS_PER_LAUNCH
MCD_ROWS_PER_LAUNCH = 128  # viettts_amd/csrc/mcd.hip; include/vtts_mcd.h: VTTS_MCD_ROWS_PER_LAUNCH (its dtw() splits by DTW_PAIRS_PER_LAUNCH)
LIMSTREAM_MAX_CHUNK = 1 << 20  # include/vtts_limstream.h: VTTS_LIMSTREAM_MAX_CHUNK
LIMSTREAM_ROWS_PER_LAUNCH = 128  # include/vtts_limstream.h: VTTS_LIMSTREAM_ROWS_PER_LAUNCH
RSSTREAM_MAX_CHUNK = 1 << 20  # include/vtts_rsstream.h: VTTS_RSSTREAM_MAX_CHUNK
RSSTREAM_ROWS_PER_LAUNCH = 128  # include/vtts_rsstream.h: VTTS_RSSTREAM_ROWS_PER_LAUNCH


class MelCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_fft", C.c_int32), ("hop", C.c_int32), ("n_mels", C.c_int32), ("fmin", C.c_float), ("fmax", C.c_float)]


class DtwCfg(C.Structure):
    _fields_ = [("n_feat", C.c_int32), ("band", C.c_int32), ("max_frames", C.c_int32)]


class McdCfg(C.Structure):
    _fields_ = [("n_mels", C.c_int32), ("n_ceps", C.c_int32), ("band", C.c_int32), ("max_frames", C.c_int32)]


class PitchCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("fmin", C.c_float), ("fmax", C.c_float), ("threshold", C.c_float)]


class LoudnessCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int32)]


class SpectralCfg(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("win", C.c_int32), ("hop", C.c_int32)]


class StftCfg(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("win", C.c_int32), ("hop", C.c_int32), ("framing", C.c_int32)]


class LimiterCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("lookahead_ms", C.c_float)]


class AudioCfg(C.Structure):
    _fields_ = [("in_rate", C.c_int32), ("out_rate", C.c_int32)]


class NatDurationCfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("lstm_dim", C.c_int32)]


class NatAcousticCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "encoder_dim", "decoder_dim", "prenet_dim", "mel_dim", "postnet_dim")]


class VttsError(RuntimeError):
    """A C-ABI call returned a negative vtts_status."""

    def __init__(self, status: int, message: str):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")


class CfgStruct(C.Structure):
    _fields_ = [
        ("num_mels", C.c_int32),
        ("upsample_initial_channel", C.c_int32),
        ("num_upsamples", C.c_int32),
        ("upsample_rates", C.c_int32 * MAX_UPSAMPLES),
        ("upsample_kernel_sizes", C.c_int32 * MAX_UPSAMPLES),
        ("num_kernels", C.c_int32),
        ("resblock_kernel_sizes", C.c_int32 * MAX_KERNELS),
        ("resblock_dilation_sizes", (C.c_int32 * 3) * MAX_KERNELS),
        ("resblock", C.c_int32),
    ]


# shorthand for the prototype table below
vp, cp, sz, i64 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int64
fp = C.POINTER(C.c_float)


def _handle_sigs(prefix: str, params: bool) -> dict:
    """The prototypes every handle shares: its lifetime's end, the packed blob and (``params``) the checkpoint arrays it takes."""
    sigs = {
        "destroy": (None, [vp]),
        "packed_bytes": (C.c_int, [vp, C.POINTER(sz)]),
        "pack": (C.c_int, [vp, vp, sz, vp]),
        "bind_packed": (C.c_int, [vp, vp, sz]),
    }
    if params:
        sigs["set_param"] = (C.c_int, [vp, cp, cp, vp, C.POINTER(i64), C.c_int])
        sigs["num_params"] = (C.c_int, [vp, C.POINTER(C.c_int)])
        sigs["param_info"] = (C.c_int, [vp, C.c_int, C.POINTER(cp), C.POINTER(cp), C.POINTER(i64), C.POINTER(C.c_int)])
    return {f"{prefix}_{name}": sig for name, sig in sigs.items()}


# Every symbol the headers under include/ declare, with its prototype: the one list (load() declares them all, and the tests check each
# header against its *_EXPORTS).
SIGS = {
    **_handle_sigs("vtts_hifigan", True),
    **_handle_sigs("vtts_nat_duration", True),
    **_handle_sigs("vtts_nat_acoustic", True),
    **_handle_sigs("vtts_mel", False),
    **_handle_sigs("vtts_audio", False),
    **_handle_sigs("vtts_disc", True),
    "vtts_abi_version": (C.c_int, []),
    "vtts_last_error": (cp, []),
    "vtts_hifigan_create": (C.c_int, [C.POINTER(CfgStruct), C.c_int, C.c_int, C.POINTER(vp)]),
    "vtts_hifigan_workspace_bytes": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(sz)]),
    "vtts_hifigan_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, sz, vp]),
    "vtts_hifigan_forward_ragged": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, sz, vp]),
    "vtts_hifigan_tap_elems": (C.c_int, [vp, cp, C.c_int, C.c_int, C.POINTER(sz)]),
    "vtts_hifigan_forward_tap": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, sz, vp, cp, vp]),
    "vtts_hifigan_run_module": (C.c_int, [vp, cp, vp, C.c_int, C.c_int, C.c_float, vp, vp, vp]),
    "vtts_hifigan_run_pair": (C.c_int, [vp, cp, vp, C.c_int, C.c_int, vp, vp]),
    "vtts_hifigan_run_resblock": (C.c_int, [vp, cp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, vp, vp]),
    "vtts_hifigan_set_option": (C.c_int, [vp, cp, i64]),
    "vtts_hifigan_get_option": (C.c_int, [vp, cp, C.POINTER(i64)]),
    "vtts_hifigan_profile_read": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(C.c_double), C.c_int]),
    "vtts_hifigan_profile_kernel": (cp, [vp]),
    "vtts_nat_duration_create": (C.c_int, [C.POINTER(NatDurationCfg), C.c_int, C.POINTER(vp)]),
    "vtts_nat_duration_workspace_bytes": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(sz)]),
    "vtts_nat_duration_forward": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, sz, vp]),
    "vtts_nat_acoustic_create": (C.c_int, [C.POINTER(NatAcousticCfg), C.c_int, C.POINTER(vp)]),
    "vtts_nat_acoustic_workspace_bytes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(sz)]),
    "vtts_nat_acoustic_set_option": (C.c_int, [vp, C.c_char_p, C.c_int]),
    "vtts_nat_acoustic_get_option": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_int)]),
    "vtts_nat_acoustic_resident_status": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "vtts_nat_acoustic_keep_masks": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
    "vtts_nat_acoustic_keep_masks_haiku": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, vp, vp]),
    "vtts_nat_acoustic_keep_masks_haiku_mode": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp]),
    "vtts_nat_acoustic_forward": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, sz, vp]),
    "vtts_nat_acoustic_forward_groups": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, sz, vp, C.c_int,
                                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vtts_nat_acoustic_wait_group": (C.c_int, [vp, C.c_int, vp]),
    "vtts_nat_acoustic_encode": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, sz, vp]),
    "vtts_nat_acoustic_forward_from_encoder": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, sz, vp, C.c_int,
                                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vtts_nat_acoustic_forward_teacher_workspace_bytes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(sz)]),
    "vtts_nat_acoustic_forward_teacher": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, sz, vp]),
    "vtts_nat_acoustic_teacher_masks_haiku": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "vtts_nat_acoustic_stream_workspace_bytes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(sz)]),
    "vtts_nat_acoustic_stream_begin": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, sz, C.c_int, vp]),
    "vtts_nat_acoustic_stream_decode": (C.c_int, [vp, C.c_int, vp]),
    "vtts_nat_acoustic_stream_finish": (C.c_int, [vp, C.c_int, C.c_int, vp]),
    "vtts_nat_acoustic_stream_end": (C.c_int, [vp]),
    "vtts_nat_acoustic_pool_workspace_bytes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(sz)]),
    "vtts_nat_acoustic_pool_open": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, sz, vp]),
    "vtts_nat_acoustic_pool_admit": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]),
    "vtts_nat_acoustic_pool_decode": (C.c_int, [vp, C.c_int, vp]),
    "vtts_nat_acoustic_pool_finish": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]),
    "vtts_nat_acoustic_pool_retire": (C.c_int, [vp, C.c_int, vp]),
    "vtts_nat_acoustic_pool_close": (C.c_int, [vp]),
    "vtts_mel_create":(C.c_int, [C.POINTER(MelCfg), C.c_int, C.POINTER(vp)]),
    "vtts_mel_num_frames": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_mel_filterbank": (C.c_int, [vp, fp]),
    "vtts_mel_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_mel_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, i64, vp, vp]),
    "vtts_audio_create": (C.c_int, [C.POINTER(AudioCfg), C.c_int, C.POINTER(vp)]),
    "vtts_audio_ratio": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vtts_audio_out_samples": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_audio_prototype": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "vtts_audio_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, C.c_int, i64, vp]),
    "vtts_disc_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "vtts_disc_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_disc_num_fmaps": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "vtts_disc_fmap_info": (C.c_int, [vp, C.c_int, C.c_int, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
    "vtts_disc_forward": (C.c_int, [vp, vp, C.c_int, i64, vp, vp, vp, vp]),
    "vtts_disc_losses": (C.c_int, [vp, vp, vp, C.c_int, i64, vp, vp]),
}


# include/vtts_dtw.h, a table of its own: SIGS stays the list of the five headers above (tests/test_handle_cpu.py checks it against their *_EXPORTS).
DTW_SIGS = {
    "vtts_dtw_create": (C.c_int, [C.POINTER(DtwCfg), C.c_int, C.POINTER(vp)]),
    "vtts_dtw_destroy": (None, [vp]),
    "vtts_dtw_workspace_bytes": (C.c_int, [vp, C.c_int, i64, i64, C.POINTER(sz)]),
    "vtts_dtw_forward": (C.c_int, [vp, vp, vp, C.c_int, i64, i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, vp, vp, sz, vp]),
}


# include/vtts_mcd.h, likewise a table of its own
MCD_SIGS = {
    "vtts_mcd_create": (C.c_int, [C.POINTER(McdCfg), C.c_int, C.POINTER(vp)]),
    "vtts_mcd_destroy": (None, [vp]),
    "vtts_mcd_basis": (C.c_int, [vp, fp]),
    "vtts_mcd_cepstra": (C.c_int, [vp, vp, C.c_int, i64, C.POINTER(C.c_int32), vp, vp]),
    "vtts_mcd_aligned_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_mcd_aligned": (C.c_int, [vp, vp, vp, C.c_int, i64, i64, C.POINTER(C.c_int32), vp, vp, i64, vp, sz, vp]),
    "vtts_mcd_dtw_workspace_bytes": (C.c_int, [vp, C.c_int, i64, i64, C.POINTER(sz)]),
    "vtts_mcd_dtw": (C.c_int, [vp, vp, vp, C.c_int, i64, i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, vp, vp, sz, vp]),
}


# include/vtts_pitch.h, likewise a table of its own
PITCH_SIGS = {
    "vtts_pitch_create": (C.c_int, [C.POINTER(PitchCfg), C.c_int, C.POINTER(vp)]),
    "vtts_pitch_destroy": (None, [vp]),
    "vtts_pitch_num_frames": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_pitch_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_pitch_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, vp, vp, i64, vp, vp]),
}


# include/vtts_loudness.h, likewise
LOUDNESS_SIGS = {
    "vtts_loudness_create": (C.c_int, [C.POINTER(LoudnessCfg), C.c_int, C.POINTER(vp)]),
    "vtts_loudness_destroy": (None, [vp]),
    "vtts_loudness_coefficients": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "vtts_loudness_num_blocks": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_loudness_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_loudness_measure": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, vp, vp, vp, vp, vp, i64, vp, sz, vp]),
    "vtts_loudness_normalize": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, vp, C.c_float, C.c_float, C.c_float, vp, C.c_int, i64,
                                          vp, vp]),
}


# include/vtts_stoi.h, likewise
STOI_SIGS = {
    "vtts_stoi_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "vtts_stoi_destroy": (None, [vp]),
    "vtts_stoi_window": (C.c_int, [vp, fp]),
    "vtts_stoi_num_frames": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_stoi_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_stoi_forward": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, sz, vp]),
}


# include/vtts_spectral.h, likewise
SPECTRAL_SIGS = {
    "vtts_spectral_create": (C.c_int, [C.POINTER(SpectralCfg), C.c_int, C.POINTER(vp)]),
    "vtts_spectral_destroy": (None, [vp]),
    "vtts_spectral_window": (C.c_int, [vp, fp]),
    "vtts_spectral_frames_per_block": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "vtts_spectral_num_frames": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_spectral_packed_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "vtts_spectral_pack": (C.c_int, [vp, vp, sz, vp]),
    "vtts_spectral_bind_packed": (C.c_int, [vp, vp, sz]),
    "vtts_spectral_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_spectral_forward": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, vp, vp, vp, vp, i64, vp, sz, vp]),
}


# include/vtts_stft.h, likewise
STFT_SIGS = {
    "vtts_stft_create": (C.c_int, [C.POINTER(StftCfg), C.c_int, C.POINTER(vp)]),
    "vtts_stft_destroy": (None, [vp]),
    "vtts_stft_window": (C.c_int, [vp, fp]),
    "vtts_stft_blocking": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vtts_stft_num_frames": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_stft_num_samples": (C.c_int, [vp, i64, C.POINTER(i64)]),
    "vtts_stft_min_envelope": (C.c_int, [vp, i64, C.POINTER(C.c_double)]),
    "vtts_stft_packed_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "vtts_stft_pack": (C.c_int, [vp, vp, sz, vp]),
    "vtts_stft_bind_packed": (C.c_int, [vp, vp, sz]),
    "vtts_stft_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, i64, vp]),
    "vtts_stft_inverse": (C.c_int, [vp, vp, C.c_int, i64, C.POINTER(C.c_int32), vp, C.c_int, i64, vp]),
    "vtts_stft_project": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, vp, vp, i64, C.c_float, vp]),
}


# include/vtts_denoise.h, likewise (created from a StftCfg)
DENOISE_SIGS = {
    "vtts_denoise_create": (C.c_int, [C.POINTER(StftCfg), C.c_int, C.POINTER(vp)]),
    "vtts_denoise_destroy": (None, [vp]),
    "vtts_denoise_blocking": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vtts_denoise_packed_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "vtts_denoise_pack": (C.c_int, [vp, vp, sz, vp]),
    "vtts_denoise_bind_packed": (C.c_int, [vp, vp, sz]),
    "vtts_denoise_apply": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, C.c_float, vp, C.c_int, i64, vp]),
}


# include/vtts_limiter.h, likewise
LIMITER_SIGS = {
    "vtts_limiter_create": (C.c_int, [C.POINTER(LimiterCfg), C.c_int, C.POINTER(vp)]),
    "vtts_limiter_destroy": (None, [vp]),
    "vtts_limiter_lookahead": (C.c_int, [vp, C.POINTER(C.c_int32)]),
    "vtts_limiter_taps": (C.c_int, [vp, fp]),
    "vtts_limiter_workspace_bytes": (C.c_int, [vp, C.c_int, i64, C.POINTER(sz)]),
    "vtts_limiter_true_peak": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, vp, vp, sz, vp]),
    "vtts_limiter_pregain": (C.c_int, [vp, vp, C.c_int, C.c_float, C.c_float, vp, vp]),
    "vtts_limiter_apply": (C.c_int, [vp, vp, C.c_int, C.c_int, i64, C.POINTER(C.c_int32), vp, C.c_float, vp, C.c_int, i64, vp, vp, vp, vp, vp, sz, vp]),
}


# include/vtts_limstream.h, likewise
i32p = C.POINTER(C.c_int32)
LIMSTREAM_SIGS = {
    "vtts_limstream_create": (C.c_int, [C.POINTER(LimiterCfg), C.c_int, C.c_int, C.c_int32, C.c_float, C.POINTER(vp)]),
    "vtts_limstream_destroy": (None, [vp]),
    "vtts_limstream_lookahead": (C.c_int, [vp, i32p]),
    "vtts_limstream_state_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "vtts_limstream_reset": (C.c_int, [vp, C.c_int, C.c_float]),
    "vtts_limstream_emit": (C.c_int, [vp, i64, i64, C.c_int32, C.c_int, C.POINTER(i64)]),
    "vtts_limstream_push": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, i32p, i64, i32p, i32p, vp, C.c_int, i32p, vp, vp]),
}


# include/vtts_rsstream.h, likewise
RSSTREAM_SIGS = {
    "vtts_rsstream_create": (C.c_int, [C.POINTER(AudioCfg), C.c_int, C.c_int, C.c_int32, C.POINTER(vp)]),
    "vtts_rsstream_destroy": (None, [vp]),
    "vtts_rsstream_ratio": (C.c_int, [vp, i32p, i32p, i32p]),
    "vtts_rsstream_state_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "vtts_rsstream_packed_bytes": (C.c_int, [vp, C.POINTER(sz)]),
    "vtts_rsstream_bind_packed": (C.c_int, [vp, vp, sz]),
    "vtts_rsstream_reset": (C.c_int, [vp, C.c_int]),
    "vtts_rsstream_cursor": (C.c_int, [vp, C.c_int, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int)]),
    "vtts_rsstream_emit": (C.c_int, [vp, i64, i64, C.c_int32, C.c_int, C.POINTER(i64)]),
    "vtts_rsstream_push": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, i32p, i64, i32p, i32p, vp, C.c_int, i32p, vp]),
}


def _exports(*prefixes: str) -> tuple:
    return tuple(name for name in SIGS if name.startswith(prefixes))


EXPORTS = _exports("vtts_abi_version", "vtts_last_error", "vtts_hifigan_")  # include/vtts_hifigan.h
NAT_EXPORTS = _exports("vtts_nat_")  # include/vtts_nat.h
MEL_EXPORTS = _exports("vtts_mel_")  # include/vtts_mel.h
DISC_EXPORTS = _exports("vtts_disc_")  # include/vtts_disc.h
AUDIO_EXPORTS = _exports("vtts_audio_")  # include/vtts_audio.h
DTW_EXPORTS = tuple(DTW_SIGS)  # include/vtts_dtw.h
MCD_EXPORTS = tuple(MCD_SIGS)  # include/vtts_mcd.h
PITCH_EXPORTS = tuple(PITCH_SIGS)  # include/vtts_pitch.h
LOUDNESS_EXPORTS = tuple(LOUDNESS_SIGS)  # include/vtts_loudness.h
STOI_EXPORTS = tuple(STOI_SIGS)  # include/vtts_stoi.h
SPECTRAL_EXPORTS = tuple(SPECTRAL_SIGS)  # include/vtts_spectral.h
STFT_EXPORTS = tuple(STFT_SIGS)  # include/vtts_stft.h
DENOISE_EXPORTS = tuple(DENOISE_SIGS)  # include/vtts_denoise.h
LIMITER_EXPORTS = tuple(LIMITER_SIGS)  # include/vtts_limiter.h
LIMSTREAM_EXPORTS = tuple(LIMSTREAM_SIGS)  # include/vtts_limstream.h
RSSTREAM_EXPORTS = tuple(RSSTREAM_SIGS)  # include/vtts_rsstream.h


def default_lib_path() -> Path:
    env = os.environ.get("VTTS_HIFIGAN_LIB")
    if env:
        return Path(env)
    return Path(__file__).resolve().parent / "lib" / "libvtts_hifigan.so"


_LIB: Optional[C.CDLL] = None
_HIP_RT = None


def _load_hip_runtime():
    """libvtts_hifigan.so carries no DT_NEEDED for the HIP runtime (csrc/build.py): bind it to the
    ONE runtime the process uses.  With PyTorch-ROCm that is torch's bundled libamdhip64.so — streams
    and device pointers handed across the C ABI come from it — otherwise the system one."""
    global _HIP_RT
    if _HIP_RT is not None:
        return _HIP_RT
    cands = []
    try:
        import torch  # noqa: F401  (loads its runtime first)

        cands.append(Path(torch.__file__).resolve().parent / "lib" / "libamdhip64.so")
    except Exception:
        pass
    cands += [Path("/opt/rocm/lib/libamdhip64.so")]
    err = None
    for c in cands:
        if c.exists():
            try:
                _HIP_RT = C.CDLL(str(c), mode=C.RTLD_GLOBAL)
                return _HIP_RT
            except OSError as e:  # pragma: no cover
                err = e
    raise OSError(f"no HIP runtime (libamdhip64) could be loaded: {err}")



def load(path=None) -> C.CDLL:
    """dlopen the HIP extension and declare prototypes.  Raises OSError if it is not built."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = Path(path) if path else default_lib_path()
    if not p.exists():
        raise OSError(
            f"HIP extension {p} not found — build it with `python -m viettts_amd.csrc.build` "
            "(there is no CPU fallback on the product path)"
        )
    _load_hip_runtime()
    lib = C.CDLL(str(p))
    for name, (res, args) in {**SIGS, **DTW_SIGS, **MCD_SIGS, **PITCH_SIGS, **LOUDNESS_SIGS, **STOI_SIGS, **SPECTRAL_SIGS, **STFT_SIGS, **DENOISE_SIGS, **LIMITER_SIGS, **LIMSTREAM_SIGS, **RSSTREAM_SIGS}.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.vtts_abi_version()
    if got != ABI_VERSION:
        raise OSError(f"{p}: ABI version {got}, this binding expects {ABI_VERSION}")
    if path is None:
        _LIB = lib
    return lib


def check(lib: C.CDLL, status: int) -> None:
    if status != 0:
        msg = lib.vtts_last_error()
        raise VttsError(status, msg.decode() if msg else "")


def make_cfg(cfg) -> CfgStruct:
    """viettts_amd.hifigan.config.HifiganConfig -> vtts_hifigan_cfg."""
    cfg.validate()
    if cfg.num_upsamples > MAX_UPSAMPLES or cfg.num_kernels > MAX_KERNELS:
        raise ValueError("architecture exceeds the C ABI's fixed array sizes")
    s = CfgStruct()
    s.num_mels = cfg.num_mels
    s.upsample_initial_channel = cfg.upsample_initial_channel
    s.num_upsamples = cfg.num_upsamples
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        s.upsample_rates[i] = int(u)
        s.upsample_kernel_sizes[i] = int(k)
    s.num_kernels = cfg.num_kernels
    for j, (k, d) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
        s.resblock_kernel_sizes[j] = int(k)
        for z in range(len(d)):
            s.resblock_dilation_sizes[j][z] = int(d[z])
    s.resblock = int(cfg.resblock)
    return s
