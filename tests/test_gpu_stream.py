"""The streaming session of the acoustic model (include/vtts_nat.h) and ``viettts_amd.streaming`` on the GPU: the streamed mel and waveform against
the un-streamed calls, bit for bit where the kernels promise it.  Synthetic checkpoints."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _nat_sessions import stream_in_windows
from viettts_amd._lib import VttsError
from viettts_amd.streaming import stream_plan, synthesize_stream

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -2


def _case(seed, L):
    """A sentence as tests/test_gpu_nat.py::_case makes it: about 3 frames per token, one word-end token of no duration."""
    rng = np.random.default_rng(seed)
    tok = list(rng.integers(0, 100, size=L))
    dur = np.abs(rng.normal(3.0, 1.5, size=L)).astype(np.float32)
    dur[rng.integers(0, L)] = 0.0
    nf = max(1, int(np.sum(dur, dtype=np.float32)))
    return tok, dur, nf


def _batch(cases):
    return [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]


# rows of 25, 12 and 3 tokens: 77, 39 and 6 frames; and rows of 32 and 3 tokens: 110 and 6 frames (frame 64 lies inside a decode call)
ROWS3 = [_case(47, 25), _case(48, 12), _case(49, 3)]
LONG2 = [_case(48, 32), _case(49, 3)]
SEEDS = [11, 12, 13]


@pytest.fixture(scope="module")
def acoustic():
    from viettts_amd.nat.acoustic import AcousticModel
    from viettts_amd.nat.synth import synthetic_acoustic_checkpoint

    m = AcousticModel(device="cuda:0")
    m.load_params(*synthetic_acoustic_checkpoint())
    yield m
    m.close()


@pytest.fixture(scope="module")
def refs(acoustic):
    """The un-streamed mels, computed once: fp32 for both batches, bf16x3 for the first."""
    assert [c[2] for c in ROWS3] == [77, 39, 6] and [c[2] for c in LONG2] == [110, 6]
    out = {"rows3": acoustic(*_batch(ROWS3), dropout_seeds=SEEDS, to_host=False), "long2": acoustic(*_batch(LONG2), dropout_seeds=SEEDS[:2], to_host=False)}
    acoustic.set_option("bf16x3", 1)
    try:
        out["rows3_x3"] = acoustic(*_batch(ROWS3), dropout_seeds=SEEDS, to_host=False)
    finally:
        acoustic.set_option("bf16x3", 0)
    return out


def _stream_in_windows(am, cases, seeds, chunk, ref):
    """The window driver all widths share (tests/_nat_sessions.py) on this module's sentences."""
    stream_in_windows(am, _batch(cases), seeds, chunk, ref)


@pytest.mark.parametrize("chunk", [1, 7, 32, 50])
def test_streamed_mel_equals_the_unstreamed_bit_for_bit(acoustic, refs, chunk):
    """Rows that end before a window (6 frames), inside its interior and inside its right halo (39 frames: windows [32, 64) and [0, 32) of chunk 32);
    windows of one 64-frame tile with <= 32 positions (chunks 1, 7) and with more (chunk 32: 52), of two tiles (chunk 50: 70); odd cursors
    (chunks 1, 7); the decoder crossing frame 64 inside one decode call (chunks 32 and 50: [42, 74) and [60, 77))."""
    _stream_in_windows(acoustic, ROWS3, SEEDS, chunk, refs["rows3"])


def test_streamed_mel_of_a_long_row_crosses_frame_64_inside_a_decode_call(acoustic, refs):
    """Fmax = 110 > 64 + 10: decode(60), then decode(110) runs frames [60, 110) — across the boundary between the gate mix's first 64 frames and the
    rest — and the windows are 60, 70 (two tiles) and 20 positions wide."""
    _stream_in_windows(acoustic, LONG2, SEEDS[:2], 50, refs["long2"])


def test_streamed_mel_bf16x3_equals_the_unstreamed_bf16x3(acoustic, refs):
    assert not torch.equal(refs["rows3_x3"], refs["rows3"])  # the option does change the bits
    acoustic.set_option("bf16x3", 1)
    try:
        _stream_in_windows(acoustic, ROWS3, SEEDS, 7, refs["rows3_x3"])
    finally:
        acoustic.set_option("bf16x3", 0)


def test_the_decoder_runs_only_as_far_as_the_plan_asks(acoustic, refs):
    """It streams: after the k-th window the cursor is the plan's ``decode_upto``, not Fmax; with 20 frames trimmed (T = n_frames - 20) the decoder
    never passes T + 10, and the kept frames are still the un-streamed ones."""
    tok, dur, n = ROWS3[0]
    T = n - 20
    plan = stream_plan(T, n, 16, 4)
    ref = refs["rows3"][:1]  # (a row does not depend on its batch; its dropout seed is its own)
    with acoustic.open_stream([tok], [dur], [n], max_window=T, dropout_seeds=SEEDS[:1]) as st:
        final = 0
        for s in plan:
            st.decode(s.decode_upto)
            if s.mel_upto > final:
                st.finish(final, s.mel_upto)
                final = s.mel_upto
            assert st.frames_decoded == s.decode_upto <= T + 10 < n
            assert torch.equal(st.mel[:, : s.mel_upto], ref[:, : s.mel_upto])
        assert final == T and st.frames_decoded == T + 10
        with pytest.raises(VttsError) as e:  # the library's cursor is the host's copy: the next window's halo has not been decoded
            st.finish(T, T + 1)
        assert e.value.status == STATE
        assert not bool(st.mel[:, T:].any())  # frames never finished stay zero


def test_session_errors_launch_nothing(acoustic, refs):
    tok, dur, n = ROWS3[1]  # 39 frames
    ref = refs["rows3"][1:2, :n]
    args = ([tok], [dur], [n])

    def refused(status, fn, *a):
        with pytest.raises(VttsError) as e:
            fn(*a)
        assert e.value.status == status, e.value

    st = acoustic.open_stream(*args, max_window=8, dropout_seeds=SEEDS[1:2])
    refused(STATE, st.finish, 0, 8)  # ahead of the cursor (0)
    st.decode(17)
    refused(STATE, st.finish, 0, 8)  # ... which must have reached 18
    st.decode(n)
    refused(INVALID, st.finish, 2, 8)  # the first window starts at 0
    refused(INVALID, st.finish, 0, 9)  # wider than max_window
    refused(INVALID, st.finish, 0, 0)  # empty
    assert not bool(st.mel.any())  # nothing has been written: the mel is what begin() made it
    st.finish(0, 8)
    refused(INVALID, st.finish, 4, 12)  # an overlap
    refused(INVALID, st.finish, 10, 14)  # a gap
    assert torch.equal(st.mel[:, :8], ref[:, :8]) and not bool(st.mel[:, 8:].any())
    st.close()
    st.close()
    refused(STATE, st.decode, n)
    refused(STATE, st.finish, 8, 16)
    # a call of the model in the middle of a session ends it and is itself unharmed
    st = acoustic.open_stream(*args, max_window=8, dropout_seeds=SEEDS[1:2])
    st.decode(5)
    assert torch.equal(acoustic(*args, dropout_seeds=SEEDS[1:2], to_host=False), ref)
    refused(STATE, st.decode, 10)
    # ... as does a second open_stream: the first object must not drive the second session
    st2 = acoustic.open_stream(*args, max_window=8, dropout_seeds=SEEDS[1:2])
    refused(STATE, st.decode, 10)
    st.close()
    st2.decode(18)
    st2.finish(0, 8)
    assert torch.equal(st2.mel[:, :8], ref[:, :8])
    st2.close()


@pytest.fixture(scope="module")
def sentence(acoustic):
    """The start of a transcript sentence, about 60 kept frames, with its frame plan and its un-streamed mel."""
    from pathlib import Path

    from viettts_amd.nat import text2mel as t2m
    from viettts_amd.nat.duration import DurationModel
    from viettts_amd.nat.synth import synthetic_duration_checkpoint, transcript_sentences

    dm = DurationModel()
    dm.load_params(*synthetic_duration_checkpoint())
    tdir = Path(__file__).parent / "golden" / "text"
    whole = min(transcript_sentences(26, tdir / "transcript.txt", tdir / "lexicon.txt"), key=len)
    # (the transcript's lines run to 120 frames and more: the shortest line's prefixes, each closed by the silence token every sentence ends with)
    sents = [list(whole[:k]) + [t2m.FLAGS.sil_index] for k in range(4, len(whole))]
    sil, seed = 0.05, 7
    _, nfr, trail = t2m.frame_plan(sents, dm(sents), sil)
    i = min(range(len(sents)), key=lambda k: (abs(nfr[k] - trail[k] - 60), k))
    fr, n, tr = t2m.frame_plan([sents[i]], dm([sents[i]]), sil)
    T = n[0] - tr[0]
    assert 40 <= T <= 90 and tr[0] > 0, (T, n, tr)  # long enough for four chunks of 16, and a trailing silence that is trimmed
    mel = acoustic([sents[i]], [fr[0]], [n[0]], dropout_seeds=[seed], to_host=False)[0, :T].contiguous()
    yield {"tokens": sents[i], "dm": dm, "sil": sil, "seed": seed, "T": T, "n": n[0], "mel": mel}
    dm.close()


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3", "f32"])
def test_streamed_waveform_equals_the_chunked_vocoder_on_the_unstreamed_mel(acoustic, sentence, dtype):
    """``synthesize_stream`` (chunks of 16 frames, the first of 4) against ``longform.synthesize_chunked`` on the un-streamed mel with the same chunk
    plan: bit-identical on the bf16 and bf16x3 engines; within 2e-6 on f32, the bound tests/test_gpu_nat.py holds "a sentence alone against the
    sentence in a batch" to on that engine (its first transposed convolution picks a summation order by the pass's length mod 4).  PCM16 chunks
    equal ``wavio.float_to_pcm16`` of the float chunks.  Against the un-chunked generator on the whole mel: the criteria of
    tests/test_gpu_longform.py (f32 < 5e-6, bf16 < 0.03, bf16x3 bit-identical)."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.generator import Generator
    from viettts_amd.hifigan.synth import synthetic_params
    from viettts_amd.longform import synthesize_chunked
    from viettts_amd.wavio import float_to_pcm16

    s = sentence
    gen = Generator(V1, device="cuda:0", dtype=dtype)
    gen.load_params(synthetic_params(V1, 4321, "scaled"))
    try:
        plan = stream_plan(s["T"], s["n"], 16, 4)
        kw = dict(silence_duration=s["sil"], dropout_seed=s["seed"], chunk_frames=16, first_chunk_frames=4)
        info = {}
        chunks = [c.copy() for c in synthesize_stream(s["tokens"], s["dm"], acoustic, gen, info=info, **kw)]
        assert [c.shape for c in chunks] == [(256 * (p.chunk.t1 - p.chunk.t0),) for p in plan] and all(c.dtype == np.float32 for c in chunks)
        assert info["frames"] == s["T"] and info["samples"] == 256 * s["T"] and info["frames_decoded_at_first_chunk"] == plan[0].decode_upto < s["n"]
        got = np.concatenate(chunks)
        want = synthesize_chunked(gen, s["mel"], chunks=[p.chunk for p in plan]).cpu().numpy()
        full = gen(s["mel"][None])[0].cpu().numpy()
        d_chunked, d_full = float(np.abs(got - want).max()), float(np.abs(got - full).max())
        print(f"[{dtype}, T = {s['T']} of {s['n']} frames, {len(plan)} chunks] streamed vs chunked: {d_chunked:.3e}; vs un-chunked: {d_full:.3e}")
        assert got.shape == want.shape == (256 * s["T"],)
        if dtype == "f32":
            assert d_chunked < 2e-6 and d_full < 5e-6
        else:
            assert np.array_equal(got, want)
            assert np.array_equal(got, full) if dtype == "bf16x3" else d_full < 0.03
        pcm = list(synthesize_stream(s["tokens"], s["dm"], acoustic, gen, out_dtype="pcm16", **kw))
        assert all(p.dtype == np.int16 for p in pcm) and len(pcm) == len(chunks)
        for p, c in zip(pcm, chunks):
            assert np.array_equal(p, float_to_pcm16(c))
    finally:
        gen.close()


def test_cli_streams_a_saved_mel(tmp_path):
    """``--mel-file m.npy --stream --chunk-frames 16`` writes the plain CLI's header and length, every sample within 1 LSB of the plain CLI's (the
    CLI criterion of tests/test_gpu_longform.py), and ``--output -`` emits exactly the file's data bytes."""
    from viettts_amd.hifigan.config import V1
    from viettts_amd.hifigan.synth import synthetic_mel, synthetic_params
    from viettts_amd.hifigan.weights import save_haiku_pickle
    from viettts_amd.wavio import read_wav

    (tmp_path / "assets/hifigan").mkdir(parents=True)
    (tmp_path / "assets/infore/hifigan").mkdir(parents=True)
    (tmp_path / "assets/hifigan/config.json").write_text(open(os.path.join(REPO, "assets/hifigan/config.json")).read())
    save_haiku_pickle(tmp_path / "assets/infore/hifigan/hk_hifi.pickle", synthetic_params(V1, 4321, "scaled"))
    np.save(tmp_path / "m.npy", synthetic_mel(1, 40, 4)[0])
    env = dict(os.environ, PYTHONPATH=REPO)

    def cli(*extra):
        r = subprocess.run([sys.executable, "-m", "viettts_amd.synthesizer", "--mel-file", "m.npy", "--sample-rate", "16000", *extra], cwd=tmp_path, env=env,
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r

    cli("--output", "plain.wav")
    r = cli("--output", "s.wav", "--stream", "--chunk-frames", "16")
    assert "writing output to file s.wav" in r.stdout.decode()
    plain, streamed = (tmp_path / "plain.wav").read_bytes(), (tmp_path / "s.wav").read_bytes()
    assert streamed[:44] == plain[:44] and len(streamed) == len(plain) == 44 + 2 * 256 * 40
    (sr, a), (_, b) = read_wav(tmp_path / "plain.wav"), read_wav(tmp_path / "s.wav")
    assert sr == 16000 and np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 1
    r = cli("--output", "-", "--stream", "--chunk-frames", "16")
    assert r.stdout == streamed[44:] and b"writing output to file -" in r.stderr
