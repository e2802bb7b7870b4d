"""Streaming one sentence, what needs no GPU: the step plan, the postnet's halo constant on the fp64 oracle, the CLI's argument errors and the WAV
header a streaming writer puts in front."""
import numpy as np
import pytest

from oracle import nat_oracle as no
from viettts_amd.dist import HALO_FRAMES
from viettts_amd.streaming import POSTNET_HALO, stream_plan


@pytest.mark.parametrize("first", [None, 4])
@pytest.mark.parametrize("chunk", [1, 7, 16, 32])
def test_stream_plan_tiles_the_kept_frames_and_bounds_the_decoder(chunk, first):
    assert POSTNET_HALO == 10 and HALO_FRAMES == 13
    for T in range(1, 81):
        for n in (T, T + 3, T + 40):
            plan = stream_plan(T, n, chunk, first)
            cs = [s.chunk for s in plan]
            # the chunks tile [0, T) exactly, in order, none empty, none longer than asked
            assert cs[0].t0 == 0 and cs[-1].t1 == T and [c.index for c in cs] == list(range(len(cs)))
            for a, b in zip(cs, cs[1:]):
                assert a.t1 == b.t0
            f = min(first, T) if first is not None else min(chunk, T)
            assert cs[0].t1 == f and all(0 < c.t1 - c.t0 <= chunk for c in cs[1:])
            assert all(c.t1 - c.t0 == chunk for c in cs[1:-1])
            for s in plan:
                c = s.chunk
                # the generator's halo is dropped only at the utterance's true edges
                assert c.lo == max(0, c.t0 - 13) and c.hi == min(T, c.t1 + 13)
                assert (c.lo == c.t0) == (c.t0 == 0) and (c.hi == c.t1) == (c.t1 == T)
                assert s.mel_upto == c.hi and s.decode_upto == min(c.hi + 10, n)
            ups = [s.decode_upto for s in plan]
            assert ups == sorted(ups) and ups[-1] == min(T + 10, n) and max(ups) <= min(T + 10, n)
            assert ups[0] == min(min(T, f + 13) + 10, n)
    with pytest.raises(ValueError):
        stream_plan(5, 4, chunk, first)
    with pytest.raises(ValueError):
        stream_plan(0, 4, chunk, first)


def _postnet(P, x):
    """The postnet of oracle.nat_oracle.acoustic_inference (vietTTS/nat/model.py:113-121) on ``x [L, mel_dim]``, without the residual."""
    pre, y = "acoustic_model", x
    for i in range(5):
        cv = "conv1_d" if i == 0 else f"conv1_d_{i}"
        y = no.conv1d_same(y, P.get(f"{pre}/~/{cv}", "w"), P.get(f"{pre}/~/{cv}", "b"))
        if i < 4:
            bn = "batch_norm" if i == 0 else f"batch_norm_{i}"
            y = np.tanh(no.batchnorm_eval(y, P.get(f"{pre}/~/{bn}", "scale"), P.get(f"{pre}/~/{bn}", "offset"),
                                          P.get(f"{pre}/~/{bn}/~/mean_ema", "average", state=True), P.get(f"{pre}/~/{bn}/~/var_ema", "average", state=True)))
    return y


def test_postnet_halo_is_ten_frames_on_the_fp64_oracle():
    """5 x Conv1D(k = 5): a frame reads 5 * (5 - 1) / 2 = 10 frames per side.  A window fed with that halo (none at the true edges) reproduces the
    whole-row postnet on its interior to fp64 rounding; with 9 frames it does not.  75 random frames, windows of 1, 7, 16 and 32."""
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

    params, state = synthetic_acoustic_checkpoint()
    P = no.Params(params, state, np.float64)
    F = 75
    x = np.random.default_rng(11).normal(0.0, 1.0, size=(F, 80))
    whole = _postnet(P, x)

    def windowed(halo, w):
        out = np.empty_like(whole)
        for f0 in range(0, F, w):
            f1 = min(F, f0 + w)
            lo, hi = max(0, f0 - halo), min(F, f1 + halo)
            out[f0:f1] = _postnet(P, x[lo:hi])[f0 - lo : f1 - lo]
        return out

    for w in (1, 7, 16, 32):
        e10, e9 = np.abs(windowed(10, w) - whole).max(), np.abs(windowed(9, w) - whole).max()
        print(f"window {w}: halo 10 -> {e10:.3e}, halo 9 -> {e9:.3e}")
        assert e10 < 1e-12 and e9 > 1e-3, (w, e10, e9)


@pytest.mark.parametrize("flag", ["--resample", "--low-latency"])
def test_cli_stream_argument_errors_come_before_any_device(flag, monkeypatch, capsys):
    import viettts_amd.streaming as streaming
    from viettts_amd import synthesizer

    def boom(*a, **k):
        raise AssertionError("the stream was started")

    monkeypatch.setattr(streaming, "stream_text", boom)
    monkeypatch.setattr(streaming, "stream_mel", boom)
    with pytest.raises(SystemExit) as e:
        synthesizer.main(["--text", "xin chào", "--stream", flag, "--sample-rate", "8000"])
    assert e.value.code == 2 and "--stream with " + flag in capsys.readouterr().err


def test_streamed_wav_header_equals_the_writers(tmp_path):
    from viettts_amd.wavio import wav_header_pcm16, write_wav_pcm16

    for n, sr in ((0, 16000), (1, 16000), (256 * 61, 22050)):
        pcm = (np.arange(n) % 251 - 125).astype(np.int16)
        write_wav_pcm16(tmp_path / "a.wav", pcm, sr)
        b = (tmp_path / "a.wav").read_bytes()
        assert b[:44] == wav_header_pcm16(n, sr) and len(b) == 44 + 2 * n
